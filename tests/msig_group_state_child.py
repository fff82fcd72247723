"""Child process of test_msig_group_gpu.py: a fresh engine.  -4 before jjs_init; create -> call (checked against the oracle) ->
jjs_shutdown -> jjs_init: the old handle is stale (-1), a group registered anew gives the same bytes."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import msig_group_cases as gcs  # noqa: E402
import multisig_cases as mc  # noqa: E402


def main() -> None:
    import torch
    torch.cuda.init()
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    gc = gcs.group_transcripts(3, 20, seed=300, threads=16)
    gc.case.corrupt(5, 1)
    e = mc.expected(gc.case, threads=16)
    pk = np.ascontiguousarray(gc.PK)
    h = ctypes.c_uint64(0)
    assert lib.jjs_msig_group_create(pk.ctypes.data_as(ctypes.c_void_p), len(pk), ctypes.byref(h)) == -4
    assert lib.jjs_msig_group_destroy(1) == -4

    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ins = [dev(x) for x in gc.call_args()]

    def run(grp):
        got = tuple(t.cpu().numpy() for t in grp.combine(*ins))
        mc.check(gc.case, e, gcs.as_inline_outputs(gc, grp.aggregate_pk, got), "child")
        return got
    first = eng.multisig_group(gc.PK)
    got1 = run(first)
    lib.jjs_shutdown()
    assert lib.jjs_init(1) == 0
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.jjs_msig_group_combine_dev(first.handle, p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), gc.T, p(out), None, p(out), p(out), None)
    assert rc == -1, rc                                         # the handle of the engine that was shut down
    assert lib.jjs_msig_group_destroy(first.handle) == -1
    first.handle = 0
    again = eng.multisig_group(gc.PK)
    assert again.handle != 0
    got2 = run(again)
    for x, y in zip(got1, got2):
        assert (x == y).all()
    again.close()
    print("ok")


if __name__ == "__main__":
    main()

"""Child process of tests/test_engine_lifecycle_gpu.py: a fresh engine, twice over -- jjs_init, one call through every buffer the
engine grows on demand (checked against the oracle), jjs_trim, jjs_shutdown -- with jjs_memory_stats recorded behind every step.
`--lib PATH`: another in-tree build of the engine (to compare two builds step by step).  One JSON line."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import msig_group_cases as gcs  # noqa: E402
import multisig_cases as mc  # noqa: E402
from helpers import ARG_ORDER, batch_to_extended, make_batch, oracle_verify, to_wire  # noqa: E402

SMALL, PIPELINE, KEY_TABLES = 256, 20000, 65536     # a lane (<= 16 384 items); the staging pipeline; KT_MIN_ITEMS: a key pool and its memo


def main() -> None:
    import torch
    torch.cuda.init()
    from jubjub_schnorr_amd import _ffi
    if "--lib" in sys.argv:
        _ffi.select_library(sys.argv[sys.argv.index("--lib") + 1])
    import bench
    import jubjub_schnorr_amd as jjs

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    # host inputs and what the oracle says of them, once for both rounds
    mixed = make_batch("single", SMALL, seed=41, n_keys=8)
    want_mixed = oracle_verify("single", mixed)
    valid = make_batch("single", SMALL, seed=43, n_keys=8, mix=False)
    want_valid = oracle_verify("single", valid)
    tenth = make_batch("single", PIPELINE // 10, seed=42, n_keys=64)         # statuses are per item: the oracle sees a tenth, tiled
    large, want_large = {k: np.tile(v, (10, 1)) for k, v in tenth.items()}, np.tile(oracle_verify("single", tenth), 10)
    by_key = make_batch("single", SMALL, seed=44, n_keys=8, mix=False)       # eight keys; every fifth signature spoilt
    by_key["u"][::5, 0] ^= 1
    want_by_key = oracle_verify("single", by_key)
    keys, idx = np.unique(by_key["PK"], axis=0, return_inverse=True)
    keys, idx = np.ascontiguousarray(keys), idx.reshape(-1).astype(np.uint32)
    assert len(keys) == 8 and (want_by_key != 0).any() and (want_mixed != 0).any() and (want_valid == 0).all()
    group = gcs.group_transcripts(3, 2, seed=310)                             # two transcripts of one group of three
    group.case.corrupt(1, 2)
    want_group = mc.expected(group.case)
    host = lambda b: [b[k] for k in ARG_ORDER["single"]]  # noqa: E731

    eng = jjs.engine()                    # jjs_init
    lib = eng._lib

    def one_round():
        stats = []

        def step(name):
            torch.cuda.synchronize()
            stats.append([name, eng.memory_stats()])

        def same(st, want, what):
            st = st.cpu().numpy() if hasattr(st, "cpu") else st
            assert (st == want).all(), what
        same(eng.verify("single", *[dev(a) for a in host(mixed)])[0], want_mixed, "resident affine"); step("resident affine")
        same(eng.verify_wire("single", *[dev(a) for a in to_wire("single", mixed)])[0], want_mixed, "resident wire"); step("resident wire")
        same(eng.verify_ext("single", *[dev(a) for a in batch_to_extended("single", mixed)])[0], want_mixed, "resident ext"); step("resident ext")
        same(eng.verify("single", *host(mixed))[0], want_mixed, "host buffers, a lane"); step("host lane")
        same(eng.verify("single", *host(large))[0], want_large, "host buffers, the pipeline"); step("host pipeline")
        arrays, expect = bench.make_inputs(eng, "single", KEY_TABLES, 0)
        st, _ = eng.verify("single", *[arrays[k] for k in bench.ARG_ORDER["single"]])
        assert torch.equal(st, expect), "resident, key tables"
        step("key tables")
        assert stats[-1][1]["key_pools"] > 0, "a call of KT_MIN_ITEMS items allocates a key pool"
        for b, want in ((valid, want_valid), (mixed, want_mixed)):
            verdict = eng.verify_all("single", *[dev(a) for a in host(b)])
            assert int(verdict.cpu()[0]) == int((want == 0).all()), "verify_all"
        step("verify_all")
        with eng.keyset("single", keys) as ks:
            same(ks.verify(dev(idx), dev(by_key["u"]), dev(by_key["R"]), dev(by_key["m"]))[0], want_by_key, "key set")
        step("key set")
        ins = [dev(a) for a in group.call_args()]
        with eng.multisig_group(group.PK) as grp:
            got = tuple(t.cpu().numpy() for t in grp.combine(*ins))
            mc.check(group.case, want_group, gcs.as_inline_outputs(group, grp.aggregate_pk, got), "signer group")
        step("signer group")
        args = group.case.args()
        got = tuple(t.cpu().numpy() for t in eng.multisig_combine(*[dev(a) for a in args[:5]], args[5]))
        mc.check(group.case, want_group, got, "inline multisig")
        step("inline multisig")
        eng.trim()
        trimmed = eng.memory_stats()
        left = eng.keyset("single", keys)         # still registered when the engine goes down
        assert left.handle != 0
        lib.jjs_shutdown()
        return stats, trimmed, left.handle

    first, trimmed_first, old = one_round()
    assert lib.jjs_init(1) == 0
    out = (ctypes.c_uint64 * 8)()
    stale = lib.jjs_keyset_info(old, out) == -1 and lib.jjs_keyset_destroy(old) == -1     # a handle of the engine that was shut down
    second, trimmed_second, _ = one_round()
    print(json.dumps({"rounds": [first, second], "after_trim": [trimmed_first, trimmed_second], "stale_handle_rejected": bool(stale)}), flush=True)


if __name__ == "__main__":
    main()

"""Child process of test_fr_gpu.py: loads the profiling build, pins the weights' seed and runs the per-item passes of the two
verdict algorithms on the device under the cases of tests/verdict_item_cases.py -- one jjs_debug_verdict_items_dev call per
case of the three schemes, one jjs_debug_keyset_items_dev call per case of the two key sets: every scalar, every block's
partial sum, the fail word and the totals, compared byte for byte with the Python expectation.  Prints "ok" and exits 0 when
every check holds."""
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import verdict_item_cases as vic  # noqa: E402


def main() -> None:
    t0 = time.time()
    import torch
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    _ffi.check(lib.jjs_debug_pin_hash_seed(2), "jjs_debug_pin_hash_seed")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    fill = lambda n: torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    raw = lambda t, n: t.cpu().numpy()[:n].tobytes()  # noqa: E731

    calls = 0
    for scheme in vic.SCHEMES:
        kinds = {"single": 2, "double": 4, "vargen": 3}[scheme]
        queued = []
        for case in vic.verdict_cases(scheme):
            n = len(case["b"]["u"])
            room = max(case["blocks"], vic.own_grid(n))
            cols = [dev(x) if x is not None else None for x in vic.batch_columns(scheme, case["b"])]
            out = [fill(kinds * n * 32), fill(room * 64), fill(16), fill(64)]
            used = ctypes.c_uint(0)
            _ffi.check(lib.jjs_debug_verdict_items_dev(vic.SCHEME_ID[scheme], *[ptr(x) for x in cols], n, case["c"], case["blocks"],
                                                       *[ptr(x) for x in out], ctypes.byref(used), stream()), "jjs_debug_verdict_items_dev")
            assert used.value == (case["blocks"] or vic.own_grid(n)), (scheme, case["name"], used.value)
            queued.append((case, cols, out, used.value))
            calls += 1
        torch.cuda.synchronize()
        for case, _, out, used in queued:
            n = len(case["b"]["u"])
            got = {"scalars": raw(out[0], kinds * n * 32), "partial": raw(out[1], used * 64), "zu": raw(out[3], 64),
                   "fail": int(np.frombuffer(raw(out[2], 4), np.uint32)[0])}
            vic.compare((scheme, case["name"]), vic.expected(scheme, case, used), got)
        del queued
    vic.classes_populated(keysets=False)
    t1 = time.time()
    print("verdict item pass: %d calls, %.1f s" % (calls, t1 - t0))

    calls = 0
    for scheme in ("single", "double"):
        keys, _ = vic.keyset(scheme)
        n_eq = len(keys)
        with eng.keyset(scheme, *keys) as ks:
            assert ks.key_status.tolist() == [int(k == vic.KEYSET_KEYS // 2) for k in range(vic.KEYSET_KEYS)]   # the identity key is registered as not valid
            queued = []
            for case in vic.keyset_cases(scheme):
                n = len(case["idx"])
                room = max(case["blocks"], vic.own_grid(n))
                b = case["b"]
                cols = [dev(case["idx"]), dev(b["u"]), dev(b["R"]), dev(b["Rp"]) if scheme == "double" else None, dev(b["m"])]
                out = [fill(n_eq * n * 32), fill(n * 32), fill(n * 32) if n_eq > 1 else None, fill(room * 64), fill(16), fill(64)]
                used = ctypes.c_uint(0)
                _ffi.check(lib.jjs_debug_keyset_items_dev(ks.handle, *[ptr(x) for x in cols], n, case["c"], case["blocks"], *[ptr(x) for x in out],
                                                          ctypes.byref(used), stream()), "jjs_debug_keyset_items_dev")
                assert used.value == (case["blocks"] or vic.own_grid(n)), (scheme, case["name"], used.value)
                queued.append((case, cols, out, used.value))
                calls += 1
            torch.cuda.synchronize()
            for case, _, out, used in queued:
                n = len(case["idx"])
                got = {"scalars": raw(out[0], n_eq * n * 32), "a": [raw(out[1 + ci], n * 32) for ci in range(n_eq)], "partial": raw(out[3], used * 64),
                       "zu": raw(out[5], 64), "fail": int(np.frombuffer(raw(out[4], 4), np.uint32)[0])}
                vic.compare((scheme, case["name"]), vic.keyset_expected(scheme, case, used), got)
            del queued
    vic.classes_populated(keysets=True)
    print("key-set item pass: %d calls, %.1f s" % (calls, time.time() - t1))
    print("ok")


if __name__ == "__main__":
    main()

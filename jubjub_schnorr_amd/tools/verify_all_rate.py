#!/usr/bin/env python3
"""One verdict per batch (include/jjs_gpu.h jjs_verify_all_*): the verdict algorithm (batch_verdict.h, msm.h) against the
per-item path and its tally, alternating in one process on one box (profiling build: jjs_debug_force_path 0x2000 /
0x4000).  Resident calls; every round checks both verdicts.  Writes one JSON line per case.
    verify_all_rate.py [out.jsonl] [rounds] [window]
    verify_all_rate.py trace [window]     (under rocprofv3 --kernel-trace --stats: three verdicts of the 2^20 case below)
Cases:
  resident     three schemes x {unique keys, 4 096 keys} x {2^16, 2^18, 2^20} valid items: ms per call of
               each mode (median, min, max over the rounds), the ratio per-item / verdict
  bad_host     2^20 single signatures with unique keys and one bad item, host buffers with statuses (the verdict, then
               the per-item path for the statuses) against the per-item host call
The 1.3x target of the issue is unique-key single at 2^20; `window` (8-16) pins the MSM's window width."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import jubjub_schnorr_amd as jjs  # noqa: E402
from jubjub_schnorr_amd import _ffi  # noqa: E402

ORDER = {"single": ["u", "R", "PK", "m"], "double": ["u", "R", "Rp", "PK", "PKp", "m"], "vargen": ["u", "R", "PK", "Gen", "m"]}
VERDICT, PER_ITEM = 0x2000, 0x4000


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def trace(window):
    import torch
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    n = 1 << 20
    a, _ = bench.make_inputs(eng, "single", n, 0, n_keys=n, mix=False)
    cols = [a[k] for k in ORDER["single"]]
    assert lib.jjs_debug_force_path(VERDICT | (window << 16)) == 0
    for _ in range(3):
        v = eng.verify_all("single", *cols)
        torch.cuda.synchronize()
        assert int(v.cpu().view(torch.int32).item()) == 1


def main():
    import torch
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_verify_all.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    window = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    device = torch.cuda.get_device_name(0)
    lines = []

    def call(scheme, cols, mode):
        assert lib.jjs_debug_force_path(mode | (window << 16)) == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = eng.verify_all(scheme, *cols)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(v.cpu().view(torch.int32).item())

    for scheme in ("single", "double", "vargen"):
        for keys in ("unique", 4096):
            for lg in (16, 18, 20):
                n = 1 << lg
                a, _ = bench.make_inputs(eng, scheme, n, 0, n_keys=n if keys == "unique" else keys, mix=False)
                cols = [a[k] for k in ORDER[scheme]]
                for mode in (VERDICT, PER_ITEM):          # warm-up: buffers sized, tables built
                    assert call(scheme, cols, mode)[1] == 1
                t = {VERDICT: [], PER_ITEM: []}
                for _ in range(rounds):
                    for mode in (VERDICT, PER_ITEM):
                        ms, v = call(scheme, cols, mode)
                        assert v == 1, (scheme, keys, n, mode)
                        t[mode].append(ms)
                rec = {"case": "resident", "scheme": scheme, "keys": keys, "items": n, "rounds": rounds, "window": window or "by size",
                       "verdict_ms": stats(t[VERDICT]), "per_item_ms": stats(t[PER_ITEM]),
                       "speedup": round(statistics.median(t[PER_ITEM]) / statistics.median(t[VERDICT]), 3), "device": device}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del a, cols
                torch.cuda.empty_cache()

    n = 1 << 20
    a, _ = bench.make_inputs(eng, "single", n, 0, n_keys=n, mix=False)
    host = [a[k].cpu().numpy() for k in ORDER["single"]]
    host[3] = host[3].copy()
    host[3][n // 2, 0] ^= 1                      # a flipped message: status 2
    t = {VERDICT: [], PER_ITEM: []}
    for r in range(rounds + 1):
        for mode in (VERDICT, PER_ITEM):
            assert lib.jjs_debug_force_path(mode | (window << 16)) == 0
            t0 = time.perf_counter()
            ok, st = eng.verify_all("single", *host)
            ms = (time.perf_counter() - t0) * 1e3
            assert not ok and int(st[n // 2]) == 2 and int((st != 0).sum()) == 1
            if r:
                t[mode].append(ms)
    rec = {"case": "bad_host", "scheme": "single", "keys": "unique", "items": n, "rounds": rounds, "window": window or "by size",
           "verdict_then_statuses_ms": stats(t[VERDICT]), "per_item_ms": stats(t[PER_ITEM]),
           "ratio": round(statistics.median(t[VERDICT]) / statistics.median(t[PER_ITEM]), 3), "device": device}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    assert lib.jjs_debug_force_path(0) == 0
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One verdict per batch against a registered key set (include/jjs_gpu.h jjs_keyset_verify_all*): the verdict algorithm
(keyset_verdict.h) against the per-item key-set route and its tally, alternating in one process on one box (profiling
build: jjs_debug_force_path 0x2000 / 0x4000).  Resident calls; every round checks both verdicts.  One JSON line per case.
    keyset_verify_all_rate.py [out.jsonl] [rounds] [window]
    keyset_verify_all_rate.py trace [window]   (under rocprofv3 --kernel-trace --stats: three verdicts of 2^20 single items)
Cases:
  resident     three schemes x {4 096, 32 768 keys} x {2^16, 2^18, 2^20} valid items: ms per call of each route (median,
               min, max over the rounds; spread = max - min), the ratio per-item / verdict; at 4 096 keys also the inline
               verdict algorithm of jjs_verify_all_* on the same items (what the collapse bought)
  one_key      2^18 items, all on one key of a 4 096-key set
A route qualifies for the verdict algorithm when its median wins by more than the larger spread of the two sides, at both
key counts of a size, and the one-key case is not slower."""
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
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
SIGCOLS = {"single": ["u", "R", "m"], "double": ["u", "R", "Rp", "m"], "vargen": ["u", "R", "m"]}
VERDICT, PER_ITEM = 0x2000, 0x4000


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def registered(eng, scheme, n, n_keys):
    """n valid items over n_keys keys (item i under key i % n_keys), the keys registered: (set, idx, columns dict)."""
    import torch
    a, _ = bench.make_inputs(eng, scheme, n, 0, n_keys=n_keys, mix=False)
    ks = eng.keyset(scheme, *[a[k][:n_keys].cpu().numpy() for k in KEYCOLS[scheme]])
    assert (ks.key_status == 0).all()
    idx = (torch.arange(n, dtype=torch.int32) % n_keys).cuda()
    return ks, idx, a


def trace(window):
    import torch
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    ks, idx, a = registered(eng, "single", 1 << 20, 4096)
    assert lib.jjs_debug_force_path(VERDICT | (window << 16)) == 0
    for _ in range(3):
        v = ks.verify_all(idx, *[a[k] for k in SIGCOLS["single"]])
        torch.cuda.synchronize()
        assert int(v.cpu().view(torch.int32).item()) == 1
    ks.close()


def main():
    import torch
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_keyset_verify_all.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    window = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")

    def timed(fn, mode):
        assert lib.jjs_debug_force_path(mode | (window << 16)) == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(v.cpu().view(torch.int32).item())

    def measure(calls):
        """calls: name -> (fn, mode), run in turn `rounds` times after one warm-up each; every verdict must be 1."""
        t = {name: [] for name in calls}
        for r in range(rounds + 1):
            for name, (fn, mode) in calls.items():
                ms, v = timed(fn, mode)
                assert v == 1, name
                if r:
                    t[name].append(ms)
        return {name: stats(xs) for name, xs in t.items()}

    def record(rec):
        rec.update(rounds=rounds, window=window or "by size", device=device)
        rec["speedup"] = round(rec["per_item_ms"]["median"] / rec["verdict_ms"]["median"], 3)
        rec["margin_ms"] = round(rec["per_item_ms"]["median"] - rec["verdict_ms"]["median"], 4)
        rec["wins_beyond_spread"] = rec["margin_ms"] > max(rec["per_item_ms"]["spread"], rec["verdict_ms"]["spread"])
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
        f.flush()

    for scheme in ("single", "double", "vargen"):
        for n_keys in (4096, 32768):
            for lg in (16, 18, 20):
                n = 1 << lg
                ks, idx, a = registered(eng, scheme, n, n_keys)
                sigs = [a[k] for k in SIGCOLS[scheme]]
                calls = {"verdict_ms": (lambda: ks.verify_all(idx, *sigs), VERDICT), "per_item_ms": (lambda: ks.verify_all(idx, *sigs), PER_ITEM)}
                if n_keys == 4096:
                    cols = [a[k] for k in ORDER[scheme]]
                    calls["inline_verdict_ms"] = (lambda: eng.verify_all(scheme, *cols), VERDICT)
                rec = {"case": "resident", "scheme": scheme, "keys": n_keys, "items": n}
                rec.update(measure(calls))
                if n_keys == 4096:
                    rec["collapse_speedup"] = round(rec["inline_verdict_ms"]["median"] / rec["verdict_ms"]["median"], 3)
                record(rec)
                ks.close()
                del a, sigs, idx, calls
                eng.trim() if hasattr(eng, "trim") else None
                torch.cuda.empty_cache()

    # every item on one key of a 4 096-key set: key 0's 64 items of the spread batch, repeated
    for scheme in ("single", "double", "vargen"):
        n = 1 << 18
        ks, idx, a = registered(eng, scheme, n, 4096)
        sel = (torch.arange(n, device="cuda") // 4096 * 4096) % n
        sigs = [a[k][sel].contiguous() for k in SIGCOLS[scheme]]
        zero = torch.zeros(n, dtype=torch.int32, device="cuda")
        rec = {"case": "one_key", "scheme": scheme, "keys": 4096, "items": n}
        rec.update(measure({"verdict_ms": (lambda: ks.verify_all(zero, *sigs), VERDICT), "per_item_ms": (lambda: ks.verify_all(zero, *sigs), PER_ITEM)}))
        record(rec)
        ks.close()
        del a, sigs
        torch.cuda.empty_cache()
    assert lib.jjs_debug_force_path(0) == 0
    f.close()


if __name__ == "__main__":
    main()

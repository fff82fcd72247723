#!/usr/bin/env python3
"""Multisig signer groups (include/jjs_gpu.h jjs_msig_group_*) against the inline multisignature call, alternating in one
process on one box on identical resident transcripts (profiling build, for the lane-mapping A/B only: jjs_debug_force_path
0x1000 makes the share pass take the shares in the caller's order).  Every round checks every output of the group call against
the inline call's, byte for byte, and the group's aggregate key against every row of the inline agg_pk.  One JSON line per case.
    msig_group_rate.py [out.jsonl] [rounds]
    msig_group_rate.py trace n T        (under rocprofv3 --kernel-trace --stats: three inline and three group calls)
Cases: n in {2, 8, 64, 256} participants at 2^17 shares; 1 and 64 transcripts of 1 000 participants.  The transcripts are valid
ones signed on the CPU (tests/msig_group_cases.py); `distinct_shares` of them are distinct, the call repeats them.
Per case: ms per call of each route (median, min, max over the rounds; spread = max - min), shares per second at the median,
the time of jjs_msig_group_create and the group's device bytes.  The group call qualifies when its median beats the inline
call's by more than the larger spread of the two sides (DESIGN.md 5g's rule)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import jubjub_schnorr_amd as jjs  # noqa: E402
import msig_group_cases as gcs  # noqa: E402
from jubjub_schnorr_amd import _ffi  # noqa: E402

CALLER_ORDER = 0x1000
BY_PARTICIPANT_FROM = 64          # csrc/msig_group_calls.h MSIG_GROUP_BY_PARTICIPANT_FROM


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def transcripts(n, T, distinct_T):
    gc = gcs.group_transcripts(n, min(T, distinct_T), seed=900 + n, threads=16)
    reps = -(-T // gc.T)
    return (gc.tile(reps) if reps > 1 else gc).slice(0, T), gc.T * n


def resident(gc):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    a = gc.case.args()
    return [dev(x) for x in a[:5]], a[5]


def trace(n, T):
    import torch
    eng = jjs.engine()
    gc, _ = transcripts(n, T, max(1, 8192 // n))
    cols, offs = resident(gc)
    grp = eng.multisig_group(gc.PK)
    for _ in range(3):
        eng.multisig_combine(*cols, offs)
        grp.combine(cols[0], cols[2], cols[3], cols[4])
        torch.cuda.synchronize()
    grp.close()


def main():
    import torch
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]), int(sys.argv[3]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_msig_group.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")

    def timed(fn, mode):
        assert lib.jjs_debug_force_path(mode) == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, got

    cases = [(n, (1 << 17) // n, max(1, 8192 // n)) for n in (2, 8, 64, 256)] + [(1000, 1, 1), (1000, 64, 2)]
    for n, T, distinct_T in cases:
        gc, distinct = transcripts(n, T, distinct_T)
        cols, offs = resident(gc)
        z, _, R, S, m = cols
        t0 = time.perf_counter()
        grp = eng.multisig_group(gc.PK)
        create_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        again = eng.multisig_group(gc.PK)                 # the second registration: no first-use allocation or code load in it
        create_again_ms = (time.perf_counter() - t0) * 1e3
        again.close()
        calls = {"inline_ms": (lambda: eng.multisig_combine(*cols, offs), 0), "group_ms": (lambda: grp.combine(z, R, S, m), 0)}
        if T >= BY_PARTICIPANT_FROM:
            calls["group_caller_order_ms"] = (lambda: grp.combine(z, R, S, m), CALLER_ORDER)
        t = {name: [] for name in calls}
        agg = torch.from_numpy(grp.aggregate_pk).cuda()
        for r in range(rounds + 2):                       # two warm-up rounds: first-use allocations, clocks
            got = {}
            for name, (fn, mode) in calls.items():
                ms, got[name] = timed(fn, mode)
                if r >= 2:
                    t[name].append(ms)
            st, agg_rows, su, sr, ts = got["inline_ms"]
            assert bool((agg_rows == agg[None]).all()), "aggregate key"
            assert int(ts.max().item()) == 0 and bool(su.any(1).all()), "the transcripts are valid"
            for name in calls:
                if name != "inline_ms":
                    for x, y in zip(got[name], (st, su, sr, ts)):
                        assert torch.equal(x, y), (n, T, name)
        rec = {"case": "resident", "participants": n, "transcripts": T, "shares": n * T, "distinct_shares": distinct, "rounds": rounds,
               "device": device, "create_ms": round(create_ms, 3), "create_again_ms": round(create_again_ms, 3),
               "group_device_bytes": grp.info()["device_bytes"],
               "share_pass_mapping": "by participant" if T >= BY_PARTICIPANT_FROM else "caller's order"}
        rec.update({name: stats(xs) for name, xs in t.items()})
        for name in calls:
            rec[name.replace("_ms", "_shares_per_s")] = round(n * T / (rec[name]["median"] * 1e-3))
        rec["speedup"] = round(rec["inline_ms"]["median"] / rec["group_ms"]["median"], 3)
        rec["margin_ms"] = round(rec["inline_ms"]["median"] - rec["group_ms"]["median"], 4)
        rec["wins_beyond_spread"] = rec["margin_ms"] > max(rec["inline_ms"]["spread"], rec["group_ms"]["spread"])
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
        f.flush()
        grp.close()
        del cols, z, R, S, m
        eng.trim()
        torch.cuda.empty_cache()
    assert lib.jjs_debug_force_path(0) == 0
    f.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Registered key sets against the inline calls, alternating in one process on one box (include/jjs_gpu.h jjs_keyset_*).
Every round checks the statuses of both against the batch's construction.  Writes one JSON line per case.
    keyset_calls.py [out.jsonl] [rounds]
Cases (the targets are the issue's, from instruction counts; each line says whether it was met):
  repeat_across   2^17 single signatures over 2^15 registered keys, resident: keyset <= 2/3 of inline
  small           1, 64, 1 024, 16 384 items, every scheme, resident: keyset <= inline (the latency path)
  survey_8d       2^20 single signatures over 4 096 keys, resident (keyset <= inline within the spread) and from host
                  buffers (keyset < inline)
  small_threads   8 threads of 64-signature host calls: calls per second, keyset against inline"""
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import jubjub_schnorr_amd as jjs  # noqa: E402

KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}


def batch(eng, scheme, n, n_keys):
    """Resident inputs, the expected statuses, the distinct keys (host) and each item's index among them."""
    a, expect = bench.make_inputs(eng, scheme, n, 0, n_keys=n_keys)
    cat = np.concatenate([a[k].cpu().numpy() for k in KEYCOLS[scheme]], 1)
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    keys = [np.ascontiguousarray(uniq[:, 64 * i:64 * i + 64]) for i in range(len(KEYCOLS[scheme]))]
    return a, expect.cpu().numpy(), keys, inv.reshape(-1).astype(np.uint32)


def timed(fn, want):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st, _ = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    got = st.cpu().numpy() if hasattr(st, "cpu") else st
    if not np.array_equal(got, want):
        raise SystemExit(f"status mismatch ({int((got != want).sum())} items)")
    return dt


def ab(rounds, inline, keyset, want):
    """Alternating rounds after one warm-up call of each; medians and spreads in ms."""
    timed(inline, want); timed(keyset, want)
    ti, tk = [], []
    for _ in range(rounds):
        ti.append(timed(inline, want))
        tk.append(timed(keyset, want))
    return {"inline_ms": statistics.median(ti), "keyset_ms": statistics.median(tk), "inline_spread_ms": max(ti) - min(ti),
            "keyset_spread_ms": max(tk) - min(tk), "ratio": statistics.median(tk) / statistics.median(ti), "status_mismatches": 0}


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r05_keyset.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    eng = jjs.engine()
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    # 1. keys that repeat across calls, not within one
    a, want, keys, idx = batch(eng, "single", 1 << 17, 1 << 15)
    didx = torch.from_numpy(idx).cuda()
    with eng.keyset("single", keys[0]) as ks:
        r = ab(rounds, lambda: eng.verify("single", a["u"], a["R"], a["PK"], a["m"]),
               lambda: ks.verify(didx, a["u"], a["R"], a["m"]), want)
        r.update(case="repeat_across", scheme="single", items=1 << 17, keys=len(keys[0]), target="keyset <= 2/3 inline",
                 met=r["ratio"] <= 2 / 3, variant_calls=ks.info())
        emit(r)

    # 2. small resident calls
    for scheme in ("single", "double", "vargen"):
        a, want, keys, idx = batch(eng, scheme, 16384, 256)
        with eng.keyset(scheme, *keys) as ks:
            for n in (1, 64, 1024, 16384):
                sub = {k: v[:n].contiguous() for k, v in a.items()}
                di = torch.from_numpy(idx[:n].copy()).cuda()
                sig = [sub["u"]] + [sub[k] for k in RCOLS[scheme]] + [sub["m"]]
                r = ab(rounds, lambda: eng.verify(scheme, *[sub[k] for k in bench.ARG_ORDER[scheme]]),
                       lambda: ks.verify(di, *sig), want[:n])
                r.update(case="small", scheme=scheme, items=n, target="keyset <= inline", met=r["keyset_ms"] <= r["inline_ms"])
                emit(r)

    # 3. SURVEY 8(d): 2^20 single signatures over 4 096 keys, resident and from host buffers
    a, want, keys, idx = batch(eng, "single", 1 << 20, 4096)
    didx = torch.from_numpy(idx).cuda()
    host = {k: v.cpu().numpy() for k, v in a.items()}
    with eng.keyset("single", keys[0]) as ks:
        r = ab(rounds, lambda: eng.verify("single", a["u"], a["R"], a["PK"], a["m"]),
               lambda: ks.verify(didx, a["u"], a["R"], a["m"]), want)
        r.update(case="survey_8d_resident", scheme="single", items=1 << 20, keys=4096, target="keyset <= inline within the spread",
                 met=r["keyset_ms"] <= r["inline_ms"] + max(r["inline_spread_ms"], r["keyset_spread_ms"]))
        emit(r)
        r = ab(rounds, lambda: eng.verify("single", host["u"], host["R"], host["PK"], host["m"]),
               lambda: ks.verify(idx, host["u"], host["R"], host["m"]), want)
        r.update(case="survey_8d_host", scheme="single", items=1 << 20, keys=4096, target="keyset < inline", met=r["ratio"] < 1.0)
        emit(r)

        # 4. eight threads of 64-signature host calls
        n, calls, threads = 64, 40, 8

        def rate(fn):
            errors = []

            def worker(t):
                lo = (t * 4096) % (len(idx) - n)
                for _ in range(calls):
                    st, _ = fn(lo)
                    if not np.array_equal(st, want[lo:lo + n]):
                        errors.append(t)
            th = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            if errors:
                raise SystemExit("status mismatch in the threaded calls")
            return threads * calls / (time.perf_counter() - t0)
        inl = lambda lo: eng.verify("single", *[host[k][lo:lo + n] for k in bench.ARG_ORDER["single"]])  # noqa: E731
        kst = lambda lo: ks.verify(idx[lo:lo + n], host["u"][lo:lo + n], host["R"][lo:lo + n], host["m"][lo:lo + n])  # noqa: E731
        rate(inl); rate(kst)
        ri, rk = [], []
        for _ in range(3):
            ri.append(rate(inl)); rk.append(rate(kst))
        emit({"case": "small_threads", "scheme": "single", "items": n, "threads": threads, "inline_calls_per_s": statistics.median(ri),
              "keyset_calls_per_s": statistics.median(rk), "ratio": statistics.median(rk) / statistics.median(ri),
              "target": "none (measured: keyset host calls run one at a time per device)", "status_mismatches": 0})
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

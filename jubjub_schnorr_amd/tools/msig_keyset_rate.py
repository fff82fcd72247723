#!/usr/bin/env python3
"""The multisignature call against a registered key set (include/jjs_gpu.h jjs_multisig_combine_keyset[_dev]) against the inline
call, alternating in one process on one box on identical resident valid transcripts.  Every round compares every output of the
two routes, byte for byte.  One JSON line per shape.
    msig_keyset_rate.py [out.jsonl] [rounds]
Shapes: 2^17 shares at 8 participants drawn from key sets of 64 and of 4 096 keys; 2 and 64 participants at 2^17 shares (4 096
keys); one small call of 512 shares; the extended format at 8 participants; the host form at 2^17 shares.  The transcripts are
valid ones signed on the CPU (tests/msig_keyset_cases.py); `distinct_shares` of them are distinct, the call repeats them.
Per shape: ms per call of each route (median, min, max over the rounds; spread = max - min) and shares per second at the
median.  A route is called faster only when its median beats the other's by more than the larger spread of the two sides
(DESIGN.md 5g's rule): `verdict` is "keyset", "inline" or "neither"."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import jjs_oracle as o  # noqa: E402
import jjs_oracle_c as oc  # noqa: E402
import jubjub_schnorr_amd as jjs  # noqa: E402
import msig_keyset_cases as kcs  # noqa: E402
import multisig_cases as mc  # noqa: E402
from helpers import pt_bytes  # noqa: E402

THREADS = 16


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def key_pool(n_keys, seed=7):
    rng = np.random.default_rng(seed)
    sk = mc._scalars(rng, n_keys)
    return oc.scalar_mul(np.tile(pt_bytes(o.G), (n_keys, 1)), mc._fe(sk), THREADS), sk


def transcripts(keys, sk, n, shares, distinct_shares, seed):
    T, dT = shares // n, max(1, min(shares, distinct_shares) // n)
    kc = kcs.pool_transcripts([n] * dT, seed, keys, sk, threads=THREADS)
    reps = -(-T // dT)
    case = (mc.tile(kc.case, reps) if reps > 1 else kc.case).slice(0, T)
    return kcs.KsCase(case, np.tile(kc.key_idx, reps)[:T * n]), dT * n


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_msig_keyset.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    pools = {k: key_pool(k) for k in (64, 4096)}
    sets = {k: eng.keyset("single", pools[k][0]) for k in pools}
    big = 1 << 17
    shapes = [("resident", 8, big, 64, "affine"), ("resident", 8, big, 4096, "affine"), ("resident", 2, big, 4096, "affine"),
              ("resident", 64, big, 4096, "affine"), ("resident small", 8, 512, 64, "affine"), ("resident", 8, big, 4096, "ext"),
              ("host", 8, big, 4096, "affine")]
    for k, (case, n, shares, n_keys, fmt) in enumerate(shapes):
        keys, sk = pools[n_keys]
        kc, distinct = transcripts(keys, sk, n, shares, 8192, 1100 + k)
        idx, z, R, S, m, offs = kc.args()
        PK = kc.case.dirty["PK"]
        if fmt == "ext":
            PK, R, S = kcs.to_ext(PK), kcs.to_ext(R), kcs.to_ext(S)
        ks = sets[n_keys]
        if case == "host":
            calls = {"inline_ms": lambda: eng.multisig_combine(z, PK, R, S, m, offs, fmt=fmt),
                     "keyset_ms": lambda: ks.multisig_combine(idx, z, R, S, m, offs, fmt=fmt)}
        else:
            d = [dev(x) for x in (idx.view(np.int32), z, PK, R, S, m)]
            calls = {"inline_ms": lambda: eng.multisig_combine(d[1], d[2], d[3], d[4], d[5], offs, fmt=fmt),
                     "keyset_ms": lambda: ks.multisig_combine(d[0], d[1], d[3], d[4], d[5], offs, fmt=fmt)}
        t = {name: [] for name in calls}
        for r in range(rounds + 2):                       # two warm-up rounds: first-use allocations, clocks
            got = {}
            for name, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[name] = fn()
                torch.cuda.synchronize()
                if r >= 2:
                    t[name].append((time.perf_counter() - t0) * 1e3)
            a, b = got["inline_ms"], got["keyset_ms"]
            ts = a[4] if case == "host" else a[4].cpu().numpy()
            assert int(ts.max()) == 0, "the transcripts are valid"
            for x, y in zip(a, b):
                assert np.array_equal(x, y) if case == "host" else torch.equal(x, y), (case, n, shares, n_keys, fmt)
        rec = {"case": case, "format": fmt, "participants": n, "transcripts": kc.T, "shares": kc.case.n, "distinct_shares": distinct,
               "set_keys": n_keys, "rounds": rounds, "device": device}
        rec.update({name: stats(xs) for name, xs in t.items()})
        for name in calls:
            rec[name.replace("_ms", "_shares_per_s")] = round(kc.case.n / (rec[name]["median"] * 1e-3))
        rec["speedup"] = round(rec["inline_ms"]["median"] / rec["keyset_ms"]["median"], 3)
        margin = rec["inline_ms"]["median"] - rec["keyset_ms"]["median"]
        spread = max(rec["inline_ms"]["spread"], rec["keyset_ms"]["spread"])
        rec["margin_ms"] = round(margin, 4)
        rec["verdict"] = "keyset" if margin > spread else ("inline" if -margin > spread else "neither")
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
        f.flush()
        eng.trim()
        torch.cuda.empty_cache()
    for s in sets.values():
        s.close()
    f.close()


if __name__ == "__main__":
    main()

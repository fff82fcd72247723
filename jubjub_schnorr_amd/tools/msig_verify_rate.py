#!/usr/bin/env python3
"""The verifier's multisignature calls (include/jjs_gpu.h jjs_multisig_verify_dev, jjs_multisig_verify_keyset_dev) against the
only route the engine offered a verifier before them -- jjs_multisig_combine_dev on the same keys with canonical dummy shares
(z = 0, m = 0, R = S = the identity), then jjs_verify_single_dev on its agg_pk -- alternating in one process on one box on
identical resident inputs, and against jjs_oracle_c on 16 host threads.  Every round compares the aggregates and the statuses
of the two device routes, byte for byte.  One JSON line per shape.
    msig_verify_rate.py [out.jsonl] [rounds]
Shapes: key vectors of 8, 64 and 256 keys at B = 1, 64 and 4 096 vectors, the keys inline and named by index into a key set of
4 096 keys.  The vectors are valid ones signed on the CPU with the aggregate secret (tests/msig_verify_cases.py);
`distinct_vectors` of them are distinct, the call repeats them.  The oracle runs jjo_multisig_combine (all of `combine`: it has no
entry point for `aggregate_pk` alone) and jjo_verify_single on the distinct vectors; its time is scaled to B.
Per shape: ms per call of each device route (median, min, max over the rounds; spread = max - min), vectors and key rows per
second at the median.  A route is called faster only when its median beats the other's by more than the larger spread of the
two sides (DESIGN.md 5g's rule): `verdict` is "verify", "combine+verify" or "neither"."""
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
import msig_verify_cases as vc  # noqa: E402
import multisig_cases as mc  # noqa: E402
from helpers import pt_bytes  # noqa: E402

THREADS = 16
SET_KEYS = 4096
DISTINCT_ROWS = 8192


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def key_pool(n_keys, seed=7):
    rng = np.random.default_rng(seed)
    sk = mc._scalars(rng, n_keys)
    return oc.scalar_mul(np.tile(pt_bytes(o.G), (n_keys, 1)), mc._fe(sk), THREADS), sk


def vectors(keys, sk, n, B, seed):
    """B valid vectors of n keys drawn without repetition from the pool, at most DISTINCT_ROWS key rows of them distinct."""
    rng = np.random.default_rng(seed)
    dB = max(1, min(B, DISTINCT_ROWS // n))
    base = vc.build([rng.permutation(len(sk))[:n] for _ in range(dB)], seed + 1, keys, sk, THREADS)
    reps = -(-B // dB)
    t = vc.tile(base, reps) if reps > 1 else base
    return vc.VCase(t.PK[:B * n], t.key_idx[:B * n], t.offsets[:B + 1], t.u[:B], t.R[:B], t.m[:B]), base


def oracle_ms(base):
    ident = np.tile(vc.IDENT, (base.n, 1))
    z, m0 = np.zeros((base.n, 32), np.uint8), np.zeros((base.B, 32), np.uint8)
    t0 = time.perf_counter()
    agg = oc.multisig_combine(z, base.PK, ident, ident, m0, base.offs32(), threads=THREADS)[2]
    st = oc.verify_single(base.u, base.R, agg, base.m, THREADS)
    ms = (time.perf_counter() - t0) * 1e3
    assert not st.any(), "the vectors are valid"
    return ms, agg


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r12_msig_verify.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    keys, sk = key_pool(SET_KEYS)
    ks = eng.keyset("single", keys)
    k = 0
    for n in (8, 64, 256):
        for B in (1, 64, 4096):
            c, base = vectors(keys, sk, n, B, 1600 + k)
            k += 1
            o_ms, o_agg = oracle_ms(base)
            offs = c.offs32()
            PK, idx, u, R, m = dev(c.PK), dev(c.key_idx.view(np.int32)), dev(c.u), dev(c.R), dev(c.m)
            z0, m0, ident = torch.zeros_like(PK[:, :32]).contiguous(), torch.zeros_like(m), dev(np.tile(vc.IDENT, (c.n, 1)))

            def parent():
                agg = eng.multisig_combine(z0, PK, ident, ident, m0, offs)[1]
                st, tally = eng.verify("single", u, R, agg, m)
                return st, tally, agg
            for form in ("inline", "keyset"):
                new = (lambda: eng.multisig_verify(PK, offs, u, R, m)) if form == "inline" else (lambda: ks.multisig_verify(idx, offs, u, R, m))
                calls = {"combine_verify_ms": parent, "verify_ms": new}
                t = {name: [] for name in calls}
                for r in range(rounds + 2):                   # two warm-up rounds: first-use allocations, clocks
                    got = {}
                    for name, fn in calls.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got[name] = fn()
                        torch.cuda.synchronize()
                        if r >= 2:
                            t[name].append((time.perf_counter() - t0) * 1e3)
                    a, b = got["combine_verify_ms"], got["verify_ms"]
                    assert int(b[0].max()) == 0, "the vectors are valid"
                    for x, y in zip(a, b):
                        assert torch.equal(x, y), (form, n, B)
                    assert np.array_equal(b[2][:base.B].cpu().numpy(), o_agg), "the aggregates are the oracle's"
                rec = {"form": form, "keys_per_vector": n, "vectors": B, "key_rows": c.n, "distinct_vectors": base.B, "set_keys": SET_KEYS,
                       "rounds": rounds, "device": device}
                rec.update({name: stats(xs) for name, xs in t.items()})
                for name in calls:
                    rec[name.replace("_ms", "_vectors_per_s")] = round(B / (rec[name]["median"] * 1e-3))
                    rec[name.replace("_ms", "_key_rows_per_s")] = round(c.n / (rec[name]["median"] * 1e-3))
                rec["speedup"] = round(rec["combine_verify_ms"]["median"] / rec["verify_ms"]["median"], 3)
                margin = rec["combine_verify_ms"]["median"] - rec["verify_ms"]["median"]
                spread = max(rec["combine_verify_ms"]["spread"], rec["verify_ms"]["spread"])
                rec["margin_ms"] = round(margin, 4)
                rec["verdict"] = "verify" if margin > spread else ("combine+verify" if -margin > spread else "neither")
                rec["oracle_threads"] = THREADS
                rec["oracle_ms_scaled"] = round(o_ms * B / base.B, 3)
                rec["oracle_ms_on_distinct"] = round(o_ms, 3)
                rec["speedup_over_oracle"] = round(rec["oracle_ms_scaled"] / rec["verify_ms"]["median"], 2)
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                f.flush()
            eng.trim()
            torch.cuda.empty_cache()
    ks.close()
    f.close()


if __name__ == "__main__":
    main()

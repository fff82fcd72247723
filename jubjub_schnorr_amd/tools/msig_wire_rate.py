#!/usr/bin/env python3
"""The wire forms of the multisignature calls (include/jjs_gpu.h "multisignature from wire encodings") against the only route a
caller with wire bytes had before them, and against the affine call alone, alternating round by round in one process on one box
on identical resident inputs.  Per shape and form three routes are timed:
    wire_ms               (a) the wire call: jjs_multisig_combine_wire_dev, jjs_msig_group_combine_wire_dev,
                              jjs_multisig_verify_wire_dev, jjs_multisig_verify_keyset_wire_dev
    decompress_affine_ms  (b) one jjs_decompress_dev per point column, then the affine call.  (Generous to this route: the `ok`
                              columns are not folded into the statuses, which such a caller has to do itself, and the verifier's
                              u and R arrive already split into two columns.)
    affine_ms             (c) the affine call alone, on columns decoded before the clock starts
Every round compares every output of the three routes, byte for byte.  One JSON line per (form, shape).
    msig_wire_rate.py [out.jsonl] [rounds]
Shapes: n = 8, 64, 256 participants (keys per vector) at B = 1, 64, 4 096 transcripts (vectors), the shapes of msig_verify_rate.py
and msig_group_rate.py restricted to those.  Forms: "combine" (inline keys), "group" (a signer group registered from wire keys),
"verify" (inline keys) and "verify_keyset" (keys by index into a set of 4 096).  Inputs are valid transcripts and vectors signed on
the CPU (tests/msig_group_cases.py, tests/msig_verify_cases.py), all decodable -- route (b) has other statuses for undecodable
points; `distinct_rows` of the rows are distinct, the call repeats them.
Per record: ms per call of each route (median, min, max over the rounds; spread = max - min), wire_over_decompress_affine = (a)/(b)
and wire_over_affine = (a)/(c) at the medians, and `verdict_vs_decompress_affine`: "wire" or "decompress+affine" when one median
beats the other by more than the larger spread of the two sides (DESIGN.md 5g's rule), else "neither"."""
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
import msig_group_cases as gcs  # noqa: E402
import msig_verify_cases as vc  # noqa: E402
import multisig_cases as mc  # noqa: E402
from helpers import pt_bytes  # noqa: E402

THREADS = 16
SET_KEYS = 4096
DISTINCT_ROWS = 8192
ROUTES = ("wire_ms", "decompress_affine_ms", "affine_ms")


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def compress_rows(aff):
    """(n, 64) canonical affine points -> (n, 32) JubJubAffine::to_bytes."""
    out = np.ascontiguousarray(aff[:, 32:]).copy()
    out[:, 31] |= (aff[:, 0] & 1) << 7
    return out


def key_pool(n_keys, seed=7):
    rng = np.random.default_rng(seed)
    sk = mc._scalars(rng, n_keys)
    return oc.scalar_mul(np.tile(pt_bytes(o.G), (n_keys, 1)), mc._fe(sk), THREADS), sk


def transcripts(n, B):
    gc = gcs.group_transcripts(n, min(B, max(1, DISTINCT_ROWS // n)), seed=900 + n, threads=THREADS)
    reps = -(-B // gc.T)
    return (gc.tile(reps) if reps > 1 else gc).slice(0, B), gc.T * n


def vectors(keys, sk, n, B, seed):
    rng = np.random.default_rng(seed)
    dB = max(1, min(B, DISTINCT_ROWS // n))
    base = vc.build([rng.permutation(len(sk))[:n] for _ in range(dB)], seed + 1, keys, sk, THREADS)
    reps = -(-B // dB)
    t = vc.tile(base, reps) if reps > 1 else base
    return vc.VCase(t.PK[:B * n], t.key_idx[:B * n], t.offsets[:B + 1], t.u[:B], t.R[:B], t.m[:B]), base.n


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r15_msig_wire.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    assert rounds >= 7
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dec = lambda w: eng.decompress(w)[0]  # noqa: E731
    keys, sk = key_pool(SET_KEYS)
    ks = eng.keyset("single", keys)

    def measure(form, n, B, rows, distinct, calls, valid):
        t = {name: [] for name in ROUTES}
        for r in range(rounds + 2):                       # two warm-up rounds: first-use allocations, clocks
            got = {}
            for name in ROUTES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[name] = calls[name]()
                torch.cuda.synchronize()
                if r >= 2:
                    t[name].append((time.perf_counter() - t0) * 1e3)
            valid(got["wire_ms"])
            for name in ROUTES[1:]:
                for x, y in zip(got["wire_ms"], got[name]):
                    assert torch.equal(x, y), (form, n, B, name)
        rec = {"form": form, "participants": n, "transcripts": B, "rows": rows, "distinct_rows": distinct, "rounds": rounds, "device": device}
        rec.update({name: stats(xs) for name, xs in t.items()})
        a, b, c = (rec[name]["median"] for name in ROUTES)
        rec["rows_per_s_wire"] = round(rows / (a * 1e-3))
        rec["wire_over_decompress_affine"] = round(a / b, 3)
        rec["wire_over_affine"] = round(a / c, 3)
        rec["decode_share_of_wire_call"] = round(1 - c / a, 3)
        spread = max(rec["wire_ms"]["spread"], rec["decompress_affine_ms"]["spread"])
        rec["margin_vs_decompress_affine_ms"] = round(b - a, 4)
        rec["verdict_vs_decompress_affine"] = "wire" if b - a > spread else ("decompress+affine" if a - b > spread else "neither")
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
        f.flush()

    k = 0
    for n in (8, 64, 256):
        for B in (1, 64, 4096):
            # ---- the combiner's calls: inline keys, and a signer group ----
            gc, distinct = transcripts(n, B)
            a = gc.case.args()
            z, PK, R, S, m = (dev(x) for x in a[:5])
            offs = a[5]
            PKw, Rw, Sw = (dev(compress_rows(x)) for x in a[1:4])

            def valid_combine(got):
                assert int(got[-1].max().item()) == 0 and bool(got[-3].any(1).all()), "the transcripts are valid"
            measure("combine", n, B, gc.case.n, distinct,
                    {"wire_ms": lambda: eng.multisig_combine_wire(z, PKw, Rw, Sw, m, offs),
                     "decompress_affine_ms": lambda: eng.multisig_combine(z, dec(PKw), dec(Rw), dec(Sw), m, offs),
                     "affine_ms": lambda: eng.multisig_combine(z, PK, R, S, m, offs)}, valid_combine)
            with eng.multisig_group_wire(compress_rows(gc.PK)) as grp:
                measure("group", n, B, gc.case.n, distinct,
                        {"wire_ms": lambda: grp.combine_wire(z, Rw, Sw, m),
                         "decompress_affine_ms": lambda: grp.combine(z, dec(Rw), dec(Sw), m),
                         "affine_ms": lambda: grp.combine(z, R, S, m)}, valid_combine)
            del z, PK, R, S, m, PKw, Rw, Sw
            # ---- the verifier's calls: inline keys, and keys by index ----
            c, distinct = vectors(keys, sk, n, B, 1600 + k)
            k += 1
            offs = c.offs32()
            PK, idx, u, R, m = dev(c.PK), dev(c.key_idx.view(np.int32)), dev(c.u), dev(c.R), dev(c.m)
            PKw, Rw = dev(compress_rows(c.PK)), dev(compress_rows(c.R))
            sig = torch.cat([u, Rw], dim=1).contiguous()

            def valid_verify(got):
                assert int(got[0].max().item()) == 0, "the vectors are valid"
            measure("verify", n, B, c.n, distinct,
                    {"wire_ms": lambda: eng.multisig_verify_wire(PKw, offs, sig, m),
                     "decompress_affine_ms": lambda: eng.multisig_verify(dec(PKw), offs, u, dec(Rw), m),
                     "affine_ms": lambda: eng.multisig_verify(PK, offs, u, R, m)}, valid_verify)
            measure("verify_keyset", n, B, c.n, distinct,
                    {"wire_ms": lambda: ks.multisig_verify_wire(idx, offs, sig, m),
                     "decompress_affine_ms": lambda: ks.multisig_verify(idx, offs, u, dec(Rw), m),
                     "affine_ms": lambda: ks.multisig_verify(idx, offs, u, R, m)}, valid_verify)
            del PK, idx, u, R, m, PKw, Rw, sig
            eng.trim()
            torch.cuda.empty_cache()
    ks.close()
    f.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The extended-coordinate multisignature calls against the affine ones, alternating in one process on one box on the same
resident valid transcripts, and the host forms at the same sizes; then the host-side alternative the extended form replaces:
one field inversion and two products per point, normalising the same points on 16 host threads (the inversion is the CPU
build of csrc/fq_inv.h from tests/hostlib.py -- the C oracle keeps its own inversion to itself --, the products are the C
oracle's).  One JSON line per case.
    msig_ext_rate.py [out.jsonl] [rounds]
Cases: the inline call, 2^17 shares at 8 participants; the group call at 2 and 8 participants.  Every round compares every
output of the two formats, byte for byte.  Per case: ms per call (median, min, max over the rounds; spread = max - min),
shares per second at the median, and ext / affine of the medians.  No threshold: the figures are the record."""
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import jubjub_schnorr_amd as jjs  # noqa: E402
import jjs_oracle_c as oc  # noqa: E402
import hostlib as hl  # noqa: E402
import msig_group_cases as gcs  # noqa: E402

SHARES = 1 << 17
THREADS = 16


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def ext_of(aff, rng):
    """(n, 64) affine -> (n, 96) extended with a random Z per point, by the C oracle's field multiplication."""
    z = rng.integers(0, 256, (len(aff), 32), dtype=np.uint8)
    z[:, 31] &= 0x3F
    z[:, 0] |= 1
    out = np.empty((len(aff), 96), np.uint8)
    out[:, :32] = oc.fq_mul(np.ascontiguousarray(aff[:, :32]), z)
    out[:, 32:64] = oc.fq_mul(np.ascontiguousarray(aff[:, 32:]), z)
    out[:, 64:] = z
    return out


def host_normalize(cols):
    """The shim's work without the extended form: one inversion and two products per point, THREADS threads."""
    def part(args):
        col, lo, hi = args
        zi = hl.fq_inv(np.ascontiguousarray(col[lo:hi, 64:]))
        return np.concatenate([oc.fq_mul(np.ascontiguousarray(col[lo:hi, :32]), zi), oc.fq_mul(np.ascontiguousarray(col[lo:hi, 32:64]), zi)], 1)
    n = len(cols[0])
    cuts = [n * k // THREADS for k in range(THREADS + 1)]
    jobs = [(c, cuts[k], cuts[k + 1]) for c in cols for k in range(THREADS)]
    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(part, jobs))
    return [np.concatenate(parts[i * THREADS:(i + 1) * THREADS]) for i in range(len(cols))]


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_msig_ext.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    hl.load(); oc.load()                                  # built before any thread asks for them
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    rng = np.random.default_rng(10)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, got

    def measure(calls, same_as):
        t = {name: [] for name in calls}
        for r in range(rounds + 2):                       # two warm-up rounds: first-use allocations, clocks
            got = {}
            for name, fn in calls.items():
                ms, got[name] = timed(fn)
                if r >= 2:
                    t[name].append(ms)
            for name, ref in same_as.items():
                for x, y in zip(got[name], got[ref]):
                    x, y = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (x, y))
                    assert (x == y).all(), (name, ref)
        return {name: stats(xs) for name, xs in t.items()}

    for kind, n in (("inline", 8), ("group", 2), ("group", 8)):
        T = SHARES // n
        gc = gcs.group_transcripts(n, max(1, 8192 // n), seed=900 + n, threads=THREADS)
        gc = gc.tile(-(-T // gc.T)).slice(0, T)
        c = gc.case.dirty
        offs = gc.case.offsets.astype(np.uint32)
        ext = {k: ext_of(c[k], rng) for k in ("PK", "R", "S")}
        pk_ext = ext["PK"][:n]
        d = {k: dev(v) for k, v in c.items()}
        dx = {k: dev(v) for k, v in ext.items()}
        rec = {"case": kind, "participants": n, "transcripts": T, "shares": n * T, "rounds": rounds, "device": device}
        if kind == "inline":
            calls = {"affine_dev_ms": lambda: eng.multisig_combine(d["z"], d["PK"], d["R"], d["S"], d["m"], offs),
                     "ext_dev_ms": lambda: eng.multisig_combine(d["z"], dx["PK"], dx["R"], dx["S"], d["m"], offs, fmt="ext"),
                     "affine_host_ms": lambda: eng.multisig_combine(c["z"], c["PK"], c["R"], c["S"], c["m"], offs),
                     "ext_host_ms": lambda: eng.multisig_combine(c["z"], ext["PK"], ext["R"], ext["S"], c["m"], offs, fmt="ext")}
            cols = [ext["PK"], ext["R"], ext["S"]]
        else:
            ga, gx = eng.multisig_group(gc.PK), eng.multisig_group(pk_ext, fmt="ext")
            assert (ga.aggregate_pk == gx.aggregate_pk).all()
            calls = {"affine_dev_ms": lambda: ga.combine(d["z"], d["R"], d["S"], d["m"]),
                     "ext_dev_ms": lambda: gx.combine(d["z"], dx["R"], dx["S"], d["m"], fmt="ext"),
                     "affine_host_ms": lambda: ga.combine(c["z"], c["R"], c["S"], c["m"]),
                     "ext_host_ms": lambda: gx.combine(c["z"], ext["R"], ext["S"], c["m"], fmt="ext")}
            cols = [ext["R"], ext["S"]]
        rec.update(measure(calls, {"ext_dev_ms": "affine_dev_ms", "affine_host_ms": "affine_dev_ms", "ext_host_ms": "affine_dev_ms"}))
        norm_ms = []
        for r in range(3):
            t0 = time.perf_counter()
            got = host_normalize(cols)
            norm_ms.append((time.perf_counter() - t0) * 1e3)
        assert all((g == c[k]).all() for g, k in zip(got, ("PK", "R", "S")[3 - len(cols):])), "the host normalisation gives the affine columns"
        rec["host_normalize_ms"] = stats(norm_ms)
        rec["host_normalize_threads"] = THREADS
        rec["host_normalize_points"] = len(cols) * n * T
        for name in calls:
            rec[name.replace("_ms", "_shares_per_s")] = round(n * T / (rec[name]["median"] * 1e-3))
        rec["ext_over_affine_dev"] = round(rec["affine_dev_ms"]["median"] / rec["ext_dev_ms"]["median"], 4)
        rec["ext_over_affine_host"] = round(rec["affine_host_ms"]["median"] / rec["ext_host_ms"]["median"], 4)
        rec["ext_dev_vs_host_normalize_plus_affine_dev"] = round(
            (rec["host_normalize_ms"]["median"] + rec["affine_dev_ms"]["median"]) / rec["ext_dev_ms"]["median"], 2)
        if kind == "group":
            ga.close(); gx.close()
        f.write(json.dumps(rec) + "\n")
        f.flush()
        print(json.dumps(rec))
    f.close()


if __name__ == "__main__":
    main()

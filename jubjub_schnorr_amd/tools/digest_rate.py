#!/usr/bin/env python3
"""Rates of jjs_digest_dev (include/jjs_gpu.h; csrc/digest.h), one JSON line per shape into profiles/r22_digest.jsonl.
    digest_rate.py [out.jsonl] [rounds] [--parent-lib jubjub_schnorr_amd/libjjs_gpu_parent.so]
Every timed side runs in a process of its own with one library loaded, and the sides alternate round by round on one box (the
manner of scripts/ab_bench.sh): `new` is this tree's libjjs_gpu.so, `parent` the library given with --parent-lib (a build of the
parent commit inside the package directory; without it the comparators run from this tree's library, where their code is the
parent's, and the lines say "parent_lib": null), `prof` this tree's libjjs_gpu_prof.so, the only build in which a route can be
forced.  Resident inputs made on the device (canonical: the top byte below 0x40).  Before anything is timed the `new` side
compares its digests byte for byte with this tree's jjs_challenge_single_dev (a) and jjs_debug_poseidon_dev (b) on the same inputs,
and the route and order variants compare their two sides.  A process times REPS back-to-back calls of a shape between two device
synchronisations (64 calls up to 1 024 items, 16 up to 2^17, 4 beyond) and reports their mean, so that a sample of a small call
is not one launch.  Per line: ms per call (median, min, max, spread = max - min of those means over the rounds) of each side and
the ratio of the medians.
  (a) k = 5 truncated against jjs_challenge_single_dev over the same 5 elements as [R, PK, m]   n in 1, 1 024, 2^16, 2^20
  (b) k = 16 against jjs_debug_poseidon_dev                                                     the same n
  (c) the eight-lane route and the one-lane route forced in turn, k in 5, 64                     n from 1 to 2^17
  (d) ragged, len(i) = 1 + (37 i mod 131), item 7 of 1 031, 2^18 items: with the order and in input order (one-lane route);
      "flat": the same without the item of 1 031, whose 258 permutations on one lane outlast everything else in the call
  (e) oracle poseidon_any on 16 threads at the shapes of (a) and (b), on the host
"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")
NS = (1, 1024, 1 << 16, 1 << 20)
ROUTE_NS = (1, 64, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072)
FORCE_COOP, FORCE_LANE, KEEP_ORDER = 0x1000000, 0x2000000, 0x4000000


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def ragged_offsets(n, long_item=True):
    lens = 1 + (37 * np.arange(n, dtype=np.int64)) % 131
    if long_item:
        lens[7] = 1031
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), lens


def worker(side, lib_path):
    """One process, one library: times every shape of its side once and prints {"key": ..., "ms": ...} lines."""
    sys.path[:0] = [ROOT]
    import ctypes
    import torch
    from jubjub_schnorr_amd import _ffi
    if side == "parent":
        # the parent's library lacks the symbols this tree's binding asks for: the two comparators are bound by hand
        torch.cuda.init()
        raw = ctypes.CDLL(lib_path)
        for name in ("jjs_init", "jjs_challenge_single_dev", "jjs_debug_poseidon_dev"):
            getattr(raw, name).argtypes = _ffi.SIGNATURES[name]
        assert raw.jjs_init(1) == 0
        P, stream = ctypes.c_void_p, lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        class Parent:
            def challenge(self, scheme, R, PK, m):
                out = torch.empty((R.shape[0], 32), dtype=torch.uint8, device="cuda")
                assert raw.jjs_challenge_single_dev(P(R.data_ptr()), P(PK.data_ptr()), P(m.data_ptr()), R.shape[0], P(out.data_ptr()), stream()) == 0
                return out

            def debug_poseidon(self, x):
                out = torch.empty((x.shape[0], 32), dtype=torch.uint8, device="cuda")
                assert raw.jjs_debug_poseidon_dev(P(x.data_ptr()), x.shape[1], x.shape[0], P(out.data_ptr()), stream()) == 0
                return out
        eng = Parent()
    else:
        _ffi.select_library(lib_path)
        import jubjub_schnorr_amd as jjs
        eng = jjs.engine()
    g = torch.Generator(device="cuda").manual_seed(22)

    def elements(count):
        x = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda", generator=g)
        x[:, 31] &= 0x3F
        return x.contiguous()

    def timed(key, fn, n, check=None):
        out = fn()                                  # warm-up: first-use allocations
        torch.cuda.synchronize()
        if check is not None:
            check(out)
        reps = 64 if n <= 1024 else (16 if n <= 1 << 17 else 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"key": key, "ms": (time.perf_counter() - t0) * 1e3 / reps}), flush=True)

    def equals(other):
        def check(out):
            want = other()
            torch.cuda.synchronize()
            assert bool((out == want).all()), "the digests are the comparator's bytes"
        return check

    if side in ("new", "parent"):
        for n in NS:
            x5, x16 = elements(5 * n), elements(16 * n)
            rows = x5.view(n, 160)
            R, PK, m = rows[:, :64].contiguous(), rows[:, 64:128].contiguous(), rows[:, 128:].contiguous()
            if side == "new":
                timed(f"a/{n}/digest", lambda: eng.digest(x5, 5, truncated=True)[0], n, equals(lambda: eng.challenge("single", R, PK, m)))
                timed(f"b/{n}/digest", lambda: eng.digest(x16, 16)[0], n, equals(lambda: eng.debug_poseidon(x16.view(n, 16, 32))))
            else:
                timed(f"a/{n}/challenge", lambda: eng.challenge("single", R, PK, m), n)
                timed(f"b/{n}/debug_poseidon", lambda: eng.debug_poseidon(x16.view(n, 16, 32)), n)
            del x5, x16
    elif side == "prof":
        force = eng._lib.jjs_debug_force_path
        for k in (5, 64):
            for n in ROUTE_NS:
                x = elements(k * n)
                ref = {}
                for name, bits in (("lane", FORCE_LANE), ("coop", FORCE_COOP)):
                    assert force(bits) == 0

                    def same(out, name=name):
                        ref.setdefault("out", out.clone())
                        assert bool((out == ref["out"]).all()), "the routes give the same bytes"
                    timed(f"c/{k}/{n}/{name}", lambda: eng.digest(x, k)[0], n, same)
                del x
        n = 1 << 18
        for shape, long_item in (("d", True), ("d_flat", False)):
            offsets, lens = ragged_offsets(n, long_item)
            x = elements(int(offsets[-1]))
            ref = {}
            for name, bits in (("ordered", FORCE_LANE), ("input_order", FORCE_LANE | KEEP_ORDER)):
                assert force(bits) == 0

                def same(out, name=name):
                    ref.setdefault("out", out.clone())
                    assert bool((out == ref["out"]).all()), "the order changes no byte"
                timed(f"{shape}/{n}/{name}", lambda: eng.digest(x, lens)[0], n, same)
            del x
        assert force(0) == 0
    else:
        raise SystemExit(f"unknown side {side}")


def run_side(side, lib_path):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", side, lib_path], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"{side} worker failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return {r["key"]: r["ms"] for r in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{"))}


def oracle_lines(rounds):
    sys.path[:0] = [os.path.join(ROOT, "oracle")]
    import jjs_oracle_c as oc
    rng = np.random.default_rng(22)
    for variant, k in (("a", 5), ("b", 16)):
        for n in NS:
            x = rng.integers(0, 256, (n, k, 32), dtype=np.uint8)
            x[:, :, 31] &= 0x3F
            ts = []
            for _ in range(min(rounds, 3) if n <= 1 << 16 else 1):          # (2^20 items of 16: a minute a run)
                t0 = time.perf_counter()
                oc.poseidon_any(x, threads=16)
                ts.append((time.perf_counter() - t0) * 1e3)
            yield {"variant": "e", "of": variant, "k": k, "n": n, "threads": 16, "oracle_ms": stats(ts)}


def main():
    args = [a for a in sys.argv[1:]]
    parent_lib = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent_lib = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r22_digest.jsonl")
    rounds = int(args[1]) if len(args) > 1 else 5
    new_lib, prof_lib = os.path.join(PKG, "libjjs_gpu.so"), os.path.join(PKG, "libjjs_gpu_prof.so")
    t = {}
    for rnd in range(rounds):
        for side, lib in (("new", new_lib), ("parent", parent_lib or new_lib), ("prof", prof_lib)):
            for key, ms in run_side(side, lib).items():
                t.setdefault(key, []).append(ms)
    lines = []
    base = {"rounds": rounds, "parent_lib": os.path.basename(parent_lib) if parent_lib else None}
    for variant, k, other in (("a", 5, "challenge"), ("b", 16, "debug_poseidon")):
        for n in NS:
            rec = {"variant": variant, "k": k, "n": n, "truncated": variant == "a", **base,
                   "digest_ms": stats(t[f"{variant}/{n}/digest"]), other + "_ms": stats(t[f"{variant}/{n}/{other}"])}
            rec["digest_over_" + other] = round(rec["digest_ms"]["median"] / rec[other + "_ms"]["median"], 3)
            rec["digests_per_s"] = round(n / rec["digest_ms"]["median"] * 1e3)
            lines.append(rec)
    for k in (5, 64):
        for n in ROUTE_NS:
            rec = {"variant": "c", "k": k, "n": n, **base, "coop_ms": stats(t[f"c/{k}/{n}/coop"]), "lane_ms": stats(t[f"c/{k}/{n}/lane"])}
            rec["coop_over_lane"] = round(rec["coop_ms"]["median"] / rec["lane_ms"]["median"], 3)
            lines.append(rec)
    n = 1 << 18
    for shape, long_item in (("d", True), ("d_flat", False)):
        rec = {"variant": shape, "n": n, "elements": int(ragged_offsets(n, long_item)[0][-1]), "longest_item": 1031 if long_item else 131, **base,
               "ordered_ms": stats(t[f"{shape}/{n}/ordered"]), "input_order_ms": stats(t[f"{shape}/{n}/input_order"])}
        rec["ordered_over_input_order"] = round(rec["ordered_ms"]["median"] / rec["input_order_ms"]["median"], 3)
        lines.append(rec)
    lines += list(oracle_lines(rounds))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        main()

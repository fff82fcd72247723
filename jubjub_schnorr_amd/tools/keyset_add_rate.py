"""What adding keys to a live key set costs (jjs_keyset_add), written to profiles/r19_keyset_add.jsonl, one JSON
row per measurement.  Every time is a host clock around a blocking call that ends in a device synchronise; the variants of a row
alternate within every round, the first round (allocations, code objects) is not counted, and a row carries the median and the
spread (max - min) of each variant.

  (a) add against create: k in {1, 64, 4 096} keys added to a set of N in {64, 4 096, 32 768} -- in place behind
      jjs_keyset_reserve, and moving the set -- against jjs_keyset_create of the N + k keys, the only route before.  The
      expectation (an add in place costs about a create of k keys, a moving one that plus a copy of N x 204 KB) is what the rows
      test: `in_place_beats_create` false at N = 32 768, k = 64 is a finding, not a pass.
  (b) calls against a grown set and a created one: jjs_keyset_verify_dev of 1, 64 and 131 072 items (shapes of
      profiles/r05_keyset.jsonl) against a set that grew from half its keys and a set created with all of them.
  (c) no regression: the same three shapes on a never-grown set.  Run the tool with --only c in this tree and in a checkout of the
      parent commit (this file copied into it: with --only c it calls nothing the parent lacks; the parent's library cannot be
      loaded from this tree, whose bindings ask for jjs_keyset_add), alternating on one box as scripts/ab_bench.sh alternates
      bench.py, and compare the rows: scripts/keyset_add_ab.sh does all of that (--tree and --process label the rows), the order
      within a pair swapped from pair to pair.  --lib takes a variant build of THIS tree.

    python jubjub_schnorr_amd/tools/keyset_add_rate.py [--only a|b|c] [--lib other/libjjs_gpu.so] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]


def stats(ms):
    ms = ms[1:]
    return {"median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abc")
    ap.add_argument("--lib", default=None, help="another in-tree build of the engine (part c: the parent commit's)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_keyset_add.jsonl"))
    ap.add_argument("--tree", default=None, help="part c: a label for the tree the tool runs in (\"this\", \"parent\"), written to the rows")
    ap.add_argument("--process", type=int, default=None, help="part c: the number of this process among the alternating ones")
    ap.add_argument("--sizes", default="64,4096,32768")
    ap.add_argument("--adds", default="1,64,4096")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: no fall-back"
    torch.cuda.set_device(0)
    from jubjub_schnorr_amd import _ffi
    if args.lib:
        _ffi.select_library(args.lib)
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    sizes, adds = [int(x) for x in args.sizes.split(",")], [int(x) for x in args.adds.split(",")]
    total = max(sizes) + max(adds)
    rng = np.random.default_rng(19)
    sk = rng.integers(0, 256, (total, 32), dtype=np.uint8)
    sk[:, 31] &= 0x0D                                   # below the group order
    PK, bad = eng.public_keys(torch.from_numpy(sk).cuda())
    keys = PK.cpu().numpy()
    assert not bad.cpu().numpy().any()
    rows = []

    def emit(row):
        row.update(device=device, lib=args.lib or "in-tree", rounds=args.rounds)
        if args.tree is not None:
            row.update(tree=args.tree, process=args.process)
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if "a" in args.only and not args.lib:
        for N in sizes:
            for k in adds:
                t = {"in_place": [], "moving": [], "create_all": []}
                for _ in range(args.rounds + 1):
                    ks = eng.keyset("single", keys[:N])
                    ks.reserve(N + k)
                    ms, _ = timed(lambda: ks.add(keys[N:N + k]))
                    assert ks.growth()["relocations"] == 1 and ks.info()["keys"] == N + k
                    t["in_place"].append(ms)
                    ks.close(); eng.trim()
                    ks = eng.keyset("single", keys[:N])
                    ms, _ = timed(lambda: ks.add(keys[N:N + k]))
                    assert ks.growth()["relocations"] == 1 and ks.growth()["capacity"] >= N + k
                    t["moving"].append(ms)
                    ks.close(); eng.trim()
                    ms, ks = timed(lambda: eng.keyset("single", keys[:N + k]))
                    t["create_all"].append(ms)
                    ks.close(); eng.trim()
                row = {"part": "a", "keys": N, "added": k}
                for name, ms in t.items():
                    row[name] = stats(ms)
                row["in_place_over_create"] = round(row["in_place"]["median_ms"] / row["create_all"]["median_ms"], 4)
                row["moving_over_create"] = round(row["moving"]["median_ms"] / row["create_all"]["median_ms"], 4)
                row["in_place_beats_create"] = row["in_place"]["median_ms"] < row["create_all"]["median_ms"]
                emit(row)

    if "b" in args.only or "c" in args.only:
        N = 4096
        shapes = [1, 64, 131072]
        n_max = max(shapes)
        idx = (np.arange(n_max) % N).astype(np.int32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        rnd = rng.integers(0, 256, (n_max, 32), dtype=np.uint8); rnd[:, 31] &= 0x0D
        m = rng.integers(0, 256, (n_max, 32), dtype=np.uint8); m[:, 31] &= 0x3F
        u, R, _ = eng.sign("single", d(sk[:N][idx]), d(rnd), d(m))
        didx, dm = d(idx), d(m)
        created = eng.keyset("single", keys[:N])
        sets = {"created": created}
        if "b" in args.only and not args.lib:
            grown = eng.keyset("single", keys[:N // 2])
            grown.add(keys[N // 2:N])
            sets["grown"] = grown
        for n in shapes:
            t = {name: [] for name in sets}
            want = None
            for _ in range(args.rounds + 1):
                for name, s in sets.items():
                    reps = 20 if n <= 64 else 5

                    def call():
                        for _ in range(reps):
                            st, _ = s.verify(didx[:n], u[:n], R[:n], dm[:n])
                        return st
                    ms, st = timed(call)
                    t[name].append(ms / reps)
                    got = st.cpu().numpy()
                    assert not got.any(), "every signature is valid"
                    assert want is None or (got == want).all()
                    want = got
            row = {"part": "b" if "grown" in sets else "c", "keys": N, "items": n}
            for name, ms in t.items():
                row[name] = stats(ms)
            if "grown" in sets:
                row["grown_over_created"] = round(row["grown"]["median_ms"] / row["created"]["median_ms"], 4)
            emit(row)
        for s in sets.values():
            s.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()

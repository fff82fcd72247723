"""What removing keys from a live key set and compacting it cost (jjs_keyset_remove, jjs_keyset_compact), written
to profiles/r20_keyset_remove.jsonl, one JSON row per measurement.  Every time is a host clock around a blocking call that ends
in a device synchronise; the variants of a row alternate within every round, the first round (allocations, code objects) is not
counted, and a row carries the median and the spread (max - min) of each variant.

  (a) remove against rebuild: jjs_keyset_remove of k in {1, 64, 4 096} keys from a set of N in {4 096, 32 768}, against
      jjs_keyset_destroy plus jjs_keyset_create of the N - k survivors, the only route before.
  (b) compact against rebuild: jjs_keyset_compact after a quarter and a half of N were removed, against the same create of the
      survivors; `gather_gb_per_s` is the bytes of the survivors' tables, read and written, over the WHOLE call's time -- a lower
      bound of what the table gather reaches (the moving add's device-to-device copy reached 2.1 TB/s).
  (c) calls against a removed-from set: jjs_keyset_verify_dev of 1, 64 and 131 072 items (no item names a removed key) against a
      set with half its keys removed, its compacted form, and a set created with the survivors.
  (d) no regression: the same three shapes on a set that was never removed from.  Run the tool with --only d in this tree and in
      a checkout of the parent commit (this file copied into it: with --only d it calls nothing the parent lacks), alternating on
      one box: scripts/keyset_remove_ab.sh does all of that (--tree and --process label the rows), the order within a pair swapped
      from pair to pair.

    python jubjub_schnorr_amd/tools/keyset_remove_rate.py [--only a|b|c|d] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]
TABLE_BYTES_PER_KEY = 43 * 33 * 144


def stats(ms):
    ms = ms[1:]
    return {"median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abc")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_keyset_remove.jsonl"))
    ap.add_argument("--tree", default=None, help="part d: a label for the tree the tool runs in (\"this\", \"parent\"), written to the rows")
    ap.add_argument("--process", type=int, default=None, help="part d: the number of this process among the alternating ones")
    ap.add_argument("--sizes", default="4096,32768")
    ap.add_argument("--removes", default="1,64,4096")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: no fall-back"
    torch.cuda.set_device(0)
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    sizes, removes = [int(x) for x in args.sizes.split(",")], [int(x) for x in args.removes.split(",")]
    total = max(sizes + [4096])
    rng = np.random.default_rng(20)
    sk = rng.integers(0, 256, (total, 32), dtype=np.uint8)
    sk[:, 31] &= 0x0D                                   # below the group order
    PK, bad = eng.public_keys(torch.from_numpy(sk).cuda())
    keys = PK.cpu().numpy()
    assert not bad.cpu().numpy().any()
    rows = []

    def emit(row):
        row.update(device=device, rounds=args.rounds)
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

    def spread_indices(N, k):
        return np.sort(np.random.default_rng(N + k).permutation(N)[:k]).astype(np.uint32)

    if "a" in args.only:
        for N in sizes:
            for k in removes:
                if k >= N:
                    continue
                gone = spread_indices(N, k)
                keep = np.ones(N, bool); keep[gone] = False
                survivors = np.ascontiguousarray(keys[:N][keep])
                t = {"remove": [], "rebuild": []}
                for _ in range(args.rounds + 1):
                    ks = eng.keyset("single", keys[:N])
                    ms, (res, n_removed) = timed(lambda: ks.remove(gone))
                    assert n_removed == k and not res.any() and ks.info()["valid_keys"] == N - k
                    t["remove"].append(ms)

                    def rebuild():
                        ks.close()
                        return eng.keyset("single", survivors)
                    ms, ks = timed(rebuild)
                    t["rebuild"].append(ms)
                    ks.close(); eng.trim()
                row = {"part": "a", "keys": N, "removed": k}
                for name, ms in t.items():
                    row[name] = stats(ms)
                row["remove_over_rebuild"] = round(row["remove"]["median_ms"] / row["rebuild"]["median_ms"], 4)
                emit(row)

    if "b" in args.only:
        for N in sizes:
            for part in (4, 2):
                k = N // part
                gone = spread_indices(N, k)
                keep = np.ones(N, bool); keep[gone] = False
                survivors = np.ascontiguousarray(keys[:N][keep])
                t = {"compact": [], "rebuild": []}
                for _ in range(args.rounds + 1):
                    ks = eng.keyset("single", keys[:N])
                    ks.remove(gone)
                    ms, m = timed(ks.compact)
                    assert ks.info()["keys"] == N - k and int((m != ks.MISS).sum()) == N - k
                    t["compact"].append(ms)

                    def rebuild():
                        ks.close()
                        return eng.keyset("single", survivors)
                    ms, ks = timed(rebuild)
                    t["rebuild"].append(ms)
                    ks.close(); eng.trim()
                row = {"part": "b", "keys": N, "removed": k}
                for name, ms in t.items():
                    row[name] = stats(ms)
                row["compact_over_rebuild"] = round(row["compact"]["median_ms"] / row["rebuild"]["median_ms"], 4)
                row["gather_gb_per_s"] = round(2 * (N - k) * TABLE_BYTES_PER_KEY / (row["compact"]["median_ms"] * 1e-3) / 1e9, 1)
                emit(row)

    if "c" in args.only or "d" in args.only:
        N = 4096
        shapes = [1, 64, 131072]
        n_max = max(shapes)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        rnd = rng.integers(0, 256, (n_max, 32), dtype=np.uint8); rnd[:, 31] &= 0x0D
        m = rng.integers(0, 256, (n_max, 32), dtype=np.uint8); m[:, 31] &= 0x3F
        dm = d(m)
        for part in [p for p in "cd" if p in args.only]:
            if part == "d":
                named = (np.arange(n_max) % N).astype(np.int32)              # the key every item names, as an index of keys[:N]
                sets = {"created": (eng.keyset("single", keys[:N]), named)}
            else:
                named = (2 * (np.arange(n_max) % (N // 2))).astype(np.int32)        # the even keys survive
                removed_from = eng.keyset("single", keys[:N])
                removed_from.remove(np.arange(1, N, 2, dtype=np.uint32))
                compacted = eng.keyset("single", keys[:N])
                compacted.remove(np.arange(1, N, 2, dtype=np.uint32))
                compacted.compact()
                sets = {"removed_from": (removed_from, named), "compacted": (compacted, named // 2),
                        "created": (eng.keyset("single", keys[:N:2]), named // 2)}
            u, R, _ = eng.sign("single", d(sk[:N][named]), d(rnd), dm)
            dev_idx = {name: d(idx) for name, (_, idx) in sets.items()}
            for n in shapes:
                t = {name: [] for name in sets}
                for _ in range(args.rounds + 1):
                    for name, (s, _) in sets.items():
                        reps = 20 if n <= 64 else 5

                        def call():
                            for _ in range(reps):
                                st, _ = s.verify(dev_idx[name][:n], u[:n], R[:n], dm[:n])
                            return st
                        ms, st = timed(call)
                        t[name].append(ms / reps)
                        assert not st.cpu().numpy().any(), "every signature is valid"
                row = {"part": part, "keys": N, "items": n}
                for name, ms in t.items():
                    row[name] = stats(ms)
                if part == "c":
                    row["removed_from_over_created"] = round(row["removed_from"]["median_ms"] / row["created"]["median_ms"], 4)
                    row["compacted_over_created"] = round(row["compacted"]["median_ms"] / row["created"]["median_ms"], 4)
                emit(row)
            for s, _ in sets.values():
                s.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()

"""The cold side of the key memo (csrc/key_tables.h step 5): two DISJOINT key sets, call after call in one slot.  Every call
then misses the memo entirely and pays its match and place kernels and the pool indirection for nothing; with --same the
calls carry one set and every call behind the first hits.  Prints one JSON line; run it alternately with --lib pointing at
the parent's build to compare (as scripts/ab_bench.sh does with bench.py).

    python jubjub_schnorr_amd/tools/key_memo_cold.py [--lib other/libjjs_gpu.so] [--scheme single] [--same] [--steps 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another in-tree build of the engine")
    ap.add_argument("--scheme", default="single", choices=["single", "double", "vargen"])
    ap.add_argument("--log2-items", type=int, default=20)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--same", action="store_true", help="one key set in every call instead of two in turn")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if args.lib:
        from jubjub_schnorr_amd import _ffi
        _ffi.select_library(args.lib)
    import bench
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    n = 1 << args.log2_items
    order = bench.ARG_ORDER[args.scheme]
    sets = []
    for rank in ((0,) if args.same else (0, 1)):          # make_inputs seeds its keys by rank: disjoint sets
        arrays, expect = bench.make_inputs(eng, args.scheme, n, rank, args.keys)
        sets.append(([arrays[k] for k in order], expect))
    exact = True
    for k in range(args.warmup):
        cols, expect = sets[k % len(sets)]
        st, _ = eng.verify(args.scheme, *cols)
        exact = exact and bool(torch.equal(st, expect))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        cols, _ = sets[(args.warmup + k) % len(sets)]
        st, _ = eng.verify(args.scheme, *cols)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    exact = exact and bool(torch.equal(st, sets[(args.warmup + args.steps - 1) % len(sets)][1]))
    print(json.dumps({"tool": "key_memo_cold", "scheme": args.scheme, "items": n, "keys_per_set": args.keys, "sets": len(sets), "steps": args.steps,
                      "ms_per_step": round(dt / args.steps * 1e3, 4), "bit_exact": exact, "lib": args.lib or "in-tree"}))


if __name__ == "__main__":
    main()

"""What registering a key set costs (jjs_keyset_create: validity, chains and window tables of every key, on the device, and
the wait for them): 2^15 single-signature keys by default, created and destroyed `--rounds` times.  Prints one JSON line; run
it alternately with --lib pointing at another build to compare.

    python jubjub_schnorr_amd/tools/keyset_create_time.py [--lib other/libjjs_gpu.so] [--log2-keys 15] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another in-tree build of the engine")
    ap.add_argument("--log2-keys", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    if args.lib:
        from jubjub_schnorr_amd import _ffi
        _ffi.select_library(args.lib)
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    n = 1 << args.log2_keys
    sk = np.random.default_rng(15).integers(0, 256, (n, 32), dtype=np.uint8)
    sk[:, 31] &= 0x0D                                   # below the group order
    PK, bad = eng.public_keys(torch.from_numpy(sk).cuda())
    keys = PK.cpu().numpy()
    assert not bad.cpu().numpy().any()
    ms = []
    for _ in range(args.rounds + 1):                     # the first round allocates: not counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ks = eng.keyset("single", keys)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert not ks.key_status.any()
        ks.close()
        eng.trim()
    ms = ms[1:]
    print(json.dumps({"tool": "keyset_create_time", "keys": n, "rounds": args.rounds, "median_ms": round(statistics.median(ms), 3),
                      "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "lib": args.lib or "in-tree"}))


if __name__ == "__main__":
    main()

"""Child process of test_keyset_lookup_gpu.py: loads the profiling build, pins the hash seed (jjs_debug_pin_hash_seed(1): a
set's lookup table is then built with seed 0) and registers the crafted sets of keyset_lookup_cases.crafted -- three keys on
the last slot of eight (the chain wraps), five colliders in 128 slots with a stranger that walks the whole chain, 64 equal
keys -- for one- and two-point sets; every lookup, resident and from host buffers, against the dict.  The keys are random
canonical coordinates, no curve points: registered (not `is_valid`) and found all the same.  A set registered after the
seed is unpinned answers alike.  Prints "ok" and exits 0 when every check holds."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import keyset_lookup_cases as kc  # noqa: E402


def main() -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def check(c, what):
        keys, queries = kc.columns(c)
        q = [x for x in queries if x is not None]
        with eng.keyset("single" if c["cols"] == 1 else "double", keys[0], keys[1]) as ks:
            assert (ks.key_status == 1).all(), (c["name"], "canonical coordinates off the curve: registered, not valid")
            got = ks.find(*[dev(x) for x in q])
            torch.cuda.synchronize()
            assert got.cpu().numpy().view(np.uint32).tolist() == c["want"].tolist(), (c["name"], what, "resident")
            assert ks.find(*q).tolist() == c["want"].tolist(), (c["name"], what, "host")

    cases = kc.crafted(1) + kc.crafted(2)
    assert lib.jjs_debug_pin_hash_seed(1) == 0
    try:
        for c in cases:
            check(c, "seed 0")
    finally:
        assert lib.jjs_debug_pin_hash_seed(0) == 0
    for c in cases:
        check(c, "a drawn seed")
    print("ok")


if __name__ == "__main__":
    main()

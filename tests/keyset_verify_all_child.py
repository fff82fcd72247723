"""Child process of test_keyset_verify_all_gpu.py: loads the profiling build, forces the verdict algorithm of
jjs_keyset_verify_all* (jjs_debug_force_path 0x2000) and checks it -- valid batches of every scheme up to 2^17 items over a
4 096-key set and one 2^20-item single batch; every item on one key at 2^17; one spoilt item per failure class, a bad
index and an invalid registered key (verdict 0, statuses byte for byte those of KeySet.verify and the oracle); cancelling
equations, cancelling torsion and an exact cofactorless equation with torsion, their keys registered; two bad items under
ONE key whose defects cancel (with random 128-bit weights this check fails spuriously with probability 2^-128); a pinned
seed (two calls agree, _dev agrees with the host call); every window width from 8 to 16 forced (w << 16) on a valid batch of
300 items and on one bad item at three positions; the set's call counters, which the verdict algorithm does not
move and the forced per-item route (0x4000) moves as KeySet.verify does.  Prints "ok" and exits 0 when every check holds."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

from helpers import ARG_ORDER, IDENT, make_batch, oracle_verify  # noqa: E402
from keyset_verify_all_cases import KEYCOLS, register_cols, same_key_pair, sig_cols  # noqa: E402
from verify_all_cases import cancelling_equations, cancelling_torsion, cofactorless_torsion, device_batch, spoil_cases  # noqa: E402


def main() -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    assert lib.jjs_debug_force_path(0x2000) == 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def dev_verdict(ks, idx, cols):
        v = ks.verify_all(dev(idx), *[dev(c) for c in cols])
        torch.cuda.synchronize()
        return int(v.cpu().view(torch.int32).item())

    def counts(ks):
        info = ks.info()
        return info["small_calls"], info["large_calls"]

    def rejected(ks, scheme, b, idx, want, name):
        sigs = sig_cols(eng, scheme, b, "affine")
        ok, st = ks.verify_all(idx, *sigs)
        per_item, _ = ks.verify(idx, *sigs)
        assert not ok, (scheme, name)
        assert st.tolist() == per_item.tolist() == want.tolist(), (scheme, name)
        assert dev_verdict(ks, idx, sigs) == 0, (scheme, name)

    # valid batches over a 4 096-key set (signed on the device), host and _dev forms; the counters do not move
    for scheme in ("single", "double", "vargen"):
        for n in (1, 65, 16385, 1 << 17) + ((1 << 20,) if scheme == "single" else ()):
            cols = [c.cpu().numpy() for c in device_batch(eng, scheme, n, 4096)]
            b = dict(zip(ARG_ORDER[scheme], cols))
            nk = min(n, 4096)
            idx = (np.arange(n) % nk).astype(np.uint32)
            with eng.keyset(scheme, *[b[k][:nk] for k in KEYCOLS[scheme]]) as ks:
                sigs = sig_cols(eng, scheme, b, "affine")
                assert dev_verdict(ks, idx, sigs) == 1, (scheme, n)
                assert ks.verify_all(idx, *sigs) == (True, None), (scheme, n)
                assert counts(ks) == (0, 0), (scheme, n, counts(ks))
                if n == 1 << 17:
                    # every item on one key: the items of key 0, repeated (a repeated item is a valid item)
                    sel = (np.arange(n) // nk * nk) % n
                    one = [c[sel] for c in sigs]
                    assert dev_verdict(ks, np.zeros(n, np.uint32), one) == 1, (scheme, "one key")
                    one[0] = one[0].copy(); one[0][n - 5, 0] ^= 1
                    assert dev_verdict(ks, np.zeros(n, np.uint32), one) == 0, (scheme, "one key, one bad u")
                    assert counts(ks) == (0, 0)
            del cols, b, sigs

    # one spoilt item per class and position, a bad index, an invalid registered key
    for scheme in ("single", "double", "vargen"):
        base = make_batch(scheme, 65, seed=41, n_keys=16, mix=False)
        for name, b in spoil_cases(scheme, base):
            keys, idx = register_cols(scheme, b)
            want = oracle_verify(scheme, b)
            assert (want != 0).sum() == 1, (scheme, name)
            with eng.keyset(scheme, *keys) as ks:
                rejected(ks, scheme, b, idx, want, name)
        keys, idx = register_cols(scheme, base)
        ident = keys[0][:1].copy(); ident[0] = IDENT
        keys = [np.concatenate([k, ident]) if i == 0 else np.concatenate([k, k[:1]]) for i, k in enumerate(keys)]
        with eng.keyset(scheme, *keys) as ks:
            assert ks.key_status[-1] == 1
            for bad, status in ((len(keys[0]), 3), (0xFFFFFFFF, 3), (len(keys[0]) - 1, 1)):
                idx2 = idx.copy(); idx2[33] = bad
                want = np.zeros(65, np.uint8); want[33] = status
                rejected(ks, scheme, base, idx2, want, f"index {bad}")

    # the constructions that defeat weaker batch checks, their keys registered; two bad items under one key
    cases = cancelling_equations() + [("single", cancelling_torsion()), ("single", cofactorless_torsion())]
    cases += [(scheme, same_key_pair(scheme)) for scheme in ("single", "double", "vargen")]
    for k, (scheme, b) in enumerate(cases):
        want = oracle_verify(scheme, b)
        assert (want != 0).any()
        keys, idx = register_cols(scheme, b)
        if k >= len(cases) - 3:
            assert len(keys[0]) == 1 and want.tolist() == [2, 2, 0, 0, 0, 0], (scheme, want)
        with eng.keyset(scheme, *keys) as ks:
            rejected(ks, scheme, b, idx, want, f"construction {k}")

    # a pinned seed: the same verdict twice, and the device call agrees with the host call
    assert lib.jjs_debug_pin_hash_seed(2) == 0
    for scheme in ("single", "double", "vargen"):
        good = make_batch(scheme, 65, seed=42, n_keys=8, mix=False)
        keys, idx = register_cols(scheme, good)
        with eng.keyset(scheme, *keys) as ks:
            for b in (good, spoil_cases(scheme, good)[0][1]):
                sigs = sig_cols(eng, scheme, b, "affine")
                v1, _ = ks.verify_all(idx, *sigs, statuses_on_failure=False)
                v2, _ = ks.verify_all(idx, *sigs, statuses_on_failure=False)
                assert v1 == v2 == bool(dev_verdict(ks, idx, sigs)) == bool((oracle_verify(scheme, b) == 0).all())
            assert counts(ks) == (0, 0)
    assert lib.jjs_debug_pin_hash_seed(0) == 0

    # every window width of the MSM forced through the real calls (by size only 8, 12, 13, 15 and 16 run above), the weights
    # pinned: a valid batch, and the same batch with one bad u at the first, middle and last item
    assert lib.jjs_debug_pin_hash_seed(2) == 0
    for scheme in ("single", "double", "vargen"):
        good = make_batch(scheme, 300, seed=43, n_keys=40, mix=False)
        bad = [b for name, b in spoil_cases(scheme, good) if name.startswith("bad_u@")]
        assert len(bad) == 3 and (oracle_verify(scheme, good) == 0).all() and all((oracle_verify(scheme, b) != 0).sum() == 1 for b in bad)
        keys, idx = register_cols(scheme, good)
        with eng.keyset(scheme, *keys) as ks:
            for w in range(8, 17):
                assert lib.jjs_debug_force_path(0x2000 | (w << 16)) == 0
                for b, want in [(good, 1)] + [(b, 0) for b in bad]:
                    sigs = sig_cols(eng, scheme, b, "affine")
                    v, _ = ks.verify_all(idx, *sigs, statuses_on_failure=False)
                    assert int(v) == want == dev_verdict(ks, idx, sigs), (scheme, w, want)
            assert counts(ks) == (0, 0)
    assert lib.jjs_debug_force_path(0x2000) == 0
    assert lib.jjs_debug_pin_hash_seed(0) == 0

    # the per-item route forced: the counters move exactly as under KeySet.verify
    assert lib.jjs_debug_force_path(0x4000) == 0
    for n in (65, 16385):
        b = make_batch("single", n, seed=45, n_keys=8, mix=False)
        keys, idx = register_cols("single", b)
        sigs = sig_cols(eng, "single", b, "affine")
        with eng.keyset("single", *keys) as ks, eng.keyset("single", *keys) as ref:
            assert ks.verify_all(idx, *sigs) == (True, None) and dev_verdict(ks, idx, sigs) == 1
            ref.verify(idx, *sigs)
            ref.verify(dev(idx), *[dev(c) for c in sigs])
            torch.cuda.synchronize()
            assert counts(ks) == counts(ref) == ((2, 0) if n <= 16384 else (0, 2)), (n, counts(ks), counts(ref))
    assert lib.jjs_debug_force_path(0) == 0
    print("ok")


if __name__ == "__main__":
    main()

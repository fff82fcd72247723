"""Child process of test_verify_all_gpu.py: loads the profiling build, forces the verdict algorithm of jjs_verify_all_*
at every size (jjs_debug_force_path 0x2000) and checks it -- valid batches of every scheme up to 2^17 items and one
2^20-item single batch with unique keys; one spoilt item per failure class at the first, middle and last position
(verdict 0, statuses byte for byte those of the inline call and the oracle); cancelling equations and cancelling
torsion; an exact cofactorless equation with torsion; a pinned seed (two calls agree, _dev agrees with the host call);
every window width from 8 to 16 forced (w << 16) on a valid batch of 300 items and on one bad item at three positions.
Prints "ok" and exits 0 when every check holds."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

from helpers import ARG_ORDER, make_batch, oracle_verify  # noqa: E402
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

    def dev_verdict(scheme, cols):
        v = eng.verify_all(scheme, *cols)
        torch.cuda.synchronize()
        return int(v.cpu().view(torch.int32).item())

    # valid batches, device columns (signed on the device), unique keys and SURVEY 8(d)'s 4 096 keys
    for scheme in ("single", "double", "vargen"):
        for n in (1, 65, 16385, 1 << 17):
            for keys in ((n, 4096) if n >= 4096 else (n,)):
                cols = device_batch(eng, scheme, n, keys)
                assert dev_verdict(scheme, cols) == 1, (scheme, n, keys)
    cols = device_batch(eng, "single", 1 << 20, 1 << 20)
    assert dev_verdict("single", cols) == 1
    host = [c.cpu().numpy() for c in cols]
    ok, st = eng.verify_all("single", *host)
    assert ok and st is None
    del cols, host

    # one spoilt item per class and position: verdict 0 and the statuses of the inline call and of the oracle
    for scheme in ("single", "double", "vargen"):
        base = make_batch(scheme, 65, seed=41, n_keys=65, mix=False)
        for name, b in spoil_cases(scheme, base):
            want = oracle_verify(scheme, b)
            assert (want != 0).sum() == 1, (scheme, name)
            cols = [b[k] for k in ARG_ORDER[scheme]]
            ok, st = eng.verify_all(scheme, *cols)
            inline, _ = eng.verify(scheme, *cols)
            assert not ok, (scheme, name)
            assert st.tolist() == inline.tolist() == want.tolist(), (scheme, name)
            assert dev_verdict(scheme, [dev(c) for c in cols]) == 0, (scheme, name)

    for scheme, b in cancelling_equations() + [("single", cancelling_torsion()), ("single", cofactorless_torsion())]:
        want = oracle_verify(scheme, b)
        assert (want != 0).any()
        ok, st = eng.verify_all(scheme, *[b[k] for k in ARG_ORDER[scheme]])
        assert not ok and st.tolist() == want.tolist(), scheme

    # a pinned seed: the same verdict twice, and the device call agrees with the host call
    assert lib.jjs_debug_pin_hash_seed(2) == 0
    for scheme in ("single", "double", "vargen"):
        good = make_batch(scheme, 65, seed=42, n_keys=8, mix=False)
        for b in (good, spoil_cases(scheme, good)[0][1]):
            cols = [b[k] for k in ARG_ORDER[scheme]]
            v1, _ = eng.verify_all(scheme, *cols, statuses_on_failure=False)
            v2, _ = eng.verify_all(scheme, *cols, statuses_on_failure=False)
            assert v1 == v2 == int(dev_verdict(scheme, [dev(c) for c in cols])) == bool((oracle_verify(scheme, b) == 0).all())
    assert lib.jjs_debug_pin_hash_seed(0) == 0

    # every window width of the MSM forced through the real calls (by size only 8, 11 and 16 run above), the weights pinned:
    # a valid batch, and the same batch with one bad u at the first, middle and last item
    assert lib.jjs_debug_pin_hash_seed(2) == 0
    for scheme in ("single", "double", "vargen"):
        good = make_batch(scheme, 300, seed=43, n_keys=300, mix=False)
        bad = [b for name, b in spoil_cases(scheme, good) if name.startswith("bad_u@")]
        assert len(bad) == 3 and (oracle_verify(scheme, good) == 0).all() and all((oracle_verify(scheme, b) != 0).sum() == 1 for b in bad)
        for w in range(8, 17):
            assert lib.jjs_debug_force_path(0x2000 | (w << 16)) == 0
            for b, want in [(good, 1)] + [(b, 0) for b in bad]:
                cols = [b[k] for k in ARG_ORDER[scheme]]
                v, _ = eng.verify_all(scheme, *cols, statuses_on_failure=False)
                assert int(v) == want == dev_verdict(scheme, [dev(c) for c in cols]), (scheme, w, want)
    assert lib.jjs_debug_force_path(0x2000) == 0
    assert lib.jjs_debug_pin_hash_seed(0) == 0
    print("ok")


if __name__ == "__main__":
    main()

"""Child process of test_sign_vargen_pt_gpu.py: loads the profiling build and forces the shared-generator route of
jjs_sign_vargen_pt* at every n (jjs_debug_force_path 0x8000) and the per-item route at every n (0x200000).  At n = 1, 63, 64,
65 and 257, under a prime-order generator, one with a torsion part, the identity and an unusable one, in every format at the
small sizes: the call forced to the shared route must equal, byte for byte, the call forced to the per-item route, the per-item
call with the generator tiled (n_gen == n never takes the shared route) and, at the first rows and the last, the oracle; the
host form and the reference's own bytes go the same way.  Prints "ok" and exits 0 when every check holds."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import jjs_oracle as o  # noqa: E402
import sign_vargen_pt_cases as vc  # noqa: E402
from helpers import to_pt  # noqa: E402


def main() -> None:
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def sign(fmt, sk, Gen, rnd, m, host=False):
        if host:
            return eng.sign_vargen_pt(sk, Gen, rnd, m, fmt=fmt)
        out = eng.sign_vargen_pt(dev(sk), dev(Gen), dev(rnd), dev(m), fmt=fmt)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]

    for which in vc.SHARED_GENERATORS + ("unusable",):
        for n in (1, 63, 64, 65, 257):
            for fmt in vc.FORMATS if n <= 64 else ("affine",):
                sk, Gen, rnd, m, p = vc.shared_call(which, n, fmt)
                assert lib.jjs_debug_force_path(0x200000) == 0
                tiled = sign(fmt, sk, np.tile(Gen, (n, 1)), rnd, m)
                plain = sign(fmt, sk, Gen, rnd, m)
                assert lib.jjs_debug_force_path(0x8000) == 0
                forced = sign(fmt, sk, Gen, rnd, m)
                for k in (0, 1, 2, 4):
                    assert (forced[k] == tiled[k]).all(), (which, n, fmt, k)
                for a, b in zip(forced, plain):
                    assert (a == b).all(), (which, n, fmt, "the two routes")
                assert forced[3].shape == (1, 64)
                if which == "unusable":
                    assert forced[4].tolist() == [3] * n and not any(x.any() for x in forced[:4]), (n, fmt)
                    continue
                assert not forced[4].any() and to_pt(forced[3][0]) == p
                for i, (wu, wR, wPK) in vc.oracle_rows(sk, p, rnd, m, sorted({0, min(1, n - 1), n - 1})).items():
                    assert (forced[0][i] == wu).all() and (forced[1][i] == wR).all() and (forced[2][i] == wPK).all(), (which, n, fmt, i)
        host = sign("ext", *vc.shared_call(which, 65, "ext")[:4], host=True)
        for a, b in zip(host, sign("ext", *vc.shared_call(which, 65, "ext")[:4])):
            assert (np.asarray(a) == b).all(), (which, "the host form")
    assert lib.jjs_debug_force_path(0x8000) == 0
    # a status-3 item among good ones, and the generator row does not depend on it
    sk, Gen, rnd, m, p = vc.shared_call("P+3T", 64)
    sk[0] = np.frombuffer(o.le32(o.R_ORDER), np.uint8)
    m[63] = np.frombuffer(o.le32(o.Q), np.uint8)
    u, R, PK, G_out, st = sign("affine", sk, Gen, rnd, m)
    assert st.tolist() == [3] + [0] * 62 + [3] and to_pt(G_out[0]) == p
    assert not (u[[0, 63]].any() or R[[0, 63]].any() or PK[[0, 63]].any()) and u[1:63].any(1).all()
    # the reference's own bytes
    with open(os.path.join(HERE, "golden", "reference_kat.json")) as f:
        k = vc.kat(json.load(f))
    key = jjs.SecretKeyVarGen.from_bytes(k["secret"])
    sig = key.sign(k["rnd"].tobytes(), k["m"].tobytes())
    assert sig.u + o.compress(to_pt(np.frombuffer(sig.R, np.uint8))) == k["signature"]
    # the tables are scratch that jjs_trim frees and the next call builds again
    before = sign("affine", *vc.shared_call("5*G", 65)[:4])
    eng.trim()
    for a, b in zip(before, sign("affine", *vc.shared_call("5*G", 65)[:4])):
        assert (a == b).all()
    print("ok")


if __name__ == "__main__":
    main()

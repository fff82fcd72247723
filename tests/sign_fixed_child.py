"""Child process of test_sign_fixed_gpu.py: loads the profiling build and forces the keyed route of jjs_sign_fixed* with one key for
the call at every n (jjs_debug_force_path 0x400000) and the per-item route at every n (0x800000).  At n = 1, 2, 64 and 257, in
both schemes, under a random key, 0, r - 1 and an unusable one: the call forced to the keyed route must equal, byte for byte, the
call forced to the per-item route, the per-item call with the key tiled (n_sk == n never takes the keyed route) and, at the first
rows and the last, the oracle; the host form and the reference's own bytes go the same way.  Prints "ok" and exits 0 when every
check holds."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import jjs_oracle as o  # noqa: E402
import sign_fixed_cases as fc  # noqa: E402
from helpers import to_pt  # noqa: E402

NAME = {False: "single", True: "double"}


def main() -> None:
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def sign(double, sk, rnd, m, host=False):
        """{name: numpy} of Engine.sign_fixed with the wire outputs"""
        if host:
            out = eng.sign_fixed(NAME[double], sk, rnd, m, wire=True)
        else:
            out = eng.sign_fixed(NAME[double], dev(sk), dev(rnd), dev(m), wire=True)
            torch.cuda.synchronize()
            out = [x.cpu().numpy() for x in out]
        return dict(zip(fc.outputs_of(double) + ("status",), out))

    for double in (False, True):
        names = fc.outputs_of(double)
        key_names = [k for k in names if k in ("PK", "PKp", "pk_w")]
        for which in fc.KEYED_KEYS:
            for n in (1, 2, 64, 257):
                sk, rnd, m = fc.keyed_call(double, which, n)
                assert lib.jjs_debug_force_path(0x800000) == 0
                tiled = sign(double, np.tile(sk, (n, 1)), rnd, m)
                plain = sign(double, sk, rnd, m)
                assert lib.jjs_debug_force_path(0x400000) == 0
                forced = sign(double, sk, rnd, m)
                for k in names + ("status",):
                    assert (forced[k] == plain[k]).all(), (double, which, n, k, "the two routes")
                    if k not in key_names:
                        assert (forced[k] == tiled[k]).all(), (double, which, n, k, "against the key tiled")
                assert all(forced[k].shape[0] == 1 for k in key_names)
                if n == 64:
                    host = sign(double, sk, rnd, m, host=True)
                    for k in names + ("status",):
                        assert (np.asarray(host[k]) == forced[k]).all(), (double, which, k, "the host form")
                if which == "unusable":
                    assert forced["status"].tolist() == [3] * n and not any(forced[k].any() for k in names), (double, n)
                    continue
                bad_first = n > 2              # keyed_call: row 0 has rnd = r
                assert forced["status"].tolist() == ([3] if bad_first else [0]) + [0] * (n - 1)
                for k, w in fc.key_rows(double, fc.keyed_key(which)).items():
                    assert (forced[k][0] == w).all(), (double, which, n, k)
                rows = [i for i in sorted({0, 1, n - 1}) if i < n and not (bad_first and i == 0)]
                for i, w in fc.oracle_rows(double, sk, rnd, m, rows).items():
                    for k in names:
                        if k not in key_names:
                            assert (forced[k][i] == w[k]).all(), (double, which, n, k, i)
        # a call of one item owns its key row: a refused item's key row is zero on both routes
        sk, rnd, m = fc.keyed_call(double, "random", 1)
        rnd[0] = np.frombuffer(o.le32(o.R_ORDER), np.uint8)
        for force in (0x400000, 0x800000):
            assert lib.jjs_debug_force_path(force) == 0
            got = sign(double, sk, rnd, m)
            assert got["status"].tolist() == [3] and not any(got[k].any() for k in names), (double, hex(force))
    assert lib.jjs_debug_force_path(0x400000) == 0
    # the reference's own bytes
    with open(os.path.join(HERE, "golden", "reference_kat.json")) as f:
        k = fc.kat(json.load(f))
    comp = lambda b: o.compress(to_pt(np.frombuffer(b, np.uint8)))  # noqa: E731
    key = jjs.SecretKey.from_bytes(k["secret"])
    sigs = jjs.SecretKey.sign_batch([(key, k["rnd"].tobytes(), k["m"].tobytes())] * 2)
    assert sigs[0] == sigs[1] and sigs[0].u + comp(sigs[0].R) == k["signature"]
    sd = jjs.SecretKey.sign_double_batch([(key, k["rnd_double"].tobytes(), k["m"].tobytes())] * 2)[1]
    assert sd.u + comp(sd.R) + comp(sd.R_prime) == k["signature_double"]
    # the key record is scratch that jjs_trim frees and the next call allocates again
    before = sign(True, *fc.keyed_call(True, "r-1", 65))
    eng.trim()
    after = sign(True, *fc.keyed_call(True, "r-1", 65))
    for name in before:
        assert (before[name] == after[name]).all(), name
    print("ok")


if __name__ == "__main__":
    main()

"""ctypes loader for tests/hostbuild/libjjs_sign_fixed_hosttest.so: csrc/sign_fixed.h and the product headers compiled for the
CPU (the recipe of sign_vargen_hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib
from msig_verify_hostlib import _aligned, _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "sign_fixed_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_sign_fixed_hosttest.so")
OUTPUTS = ("u", "R", "Rp", "PK", "PKp", "sig_w", "pk_w")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _outputs(double, n, n_sk, skip=()):
    shapes = dict(u=(n, 32), R=(n, 64), Rp=(n, 64), PK=(n_sk, 64), PKp=(n_sk, 64), sig_w=(n, 96 if double else 64),
                  pk_w=(n_sk, 64 if double else 32))
    out = {}
    for k in OUTPUTS:
        foreign = not double and k in ("Rp", "PKp")
        out[k] = None if (foreign or k in skip) else _aligned(np.full(shapes[k], 0xA5, np.uint8))
    return out


def sign(double, sk, rnd, m, route=0, skip=()):
    """One signing call; sk of n rows or of one row; route 1: the pre-pass and the keyed body.  Returns a dict of the outputs (u, R,
    Rp, PK, PKp, sig_w, pk_w: None for those in `skip` and for what the scheme does not have) and status, prefilled with 0xA5."""
    sk, rnd, m = (_aligned(x) for x in (sk, rnd, m))
    n, n_sk = len(rnd), len(sk)
    out = _outputs(double, n, n_sk, skip)
    st = np.full(n, 0xA5, np.uint8)
    rc = load().jjs_sign_fixed_host(int(bool(double)), 1, int(route), _p(sk), ctypes.c_size_t(n_sk), _p(rnd), _p(m), ctypes.c_size_t(n),
                                    *[_p(out[k]) for k in OUTPUTS], _p(st))
    assert rc == 0, rc
    out["status"] = st
    return out


def derive(double, sk, skip=()):
    """One derivation call.  Returns a dict of PK, PKp, pk_w and status, prefilled with 0xA5."""
    sk = _aligned(sk)
    n = len(sk)
    out = _outputs(double, n, n, tuple(skip) + ("u", "R", "Rp", "sig_w"))
    st = np.full(n, 0xA5, np.uint8)
    rc = load().jjs_sign_fixed_host(int(bool(double)), 0, 0, _p(sk), ctypes.c_size_t(n), None, None, ctypes.c_size_t(n),
                                    *[_p(out[k]) for k in OUTPUTS], _p(st))
    assert rc == 0, rc
    out["status"] = st
    return out

"""ctypes loader for tests/hostbuild/libjjs_sign_vargen_hosttest.so: csrc/sign_vargen.h and the product headers compiled for the
CPU (the recipe of msig_sign_hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib
from msig_verify_hostlib import _aligned, _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "sign_vargen_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_sign_vargen_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def sign(fmt_code, sk, Gen, rnd, m, route=0, lanes=3, want_pk=True, want_gen=True):
    """One signing call; route 1: the shared-generator route (Gen of one row).  Returns (u, R, PK, Gen_out, status), prefilled
    with 0xA5 (PK / Gen_out None when not asked for)."""
    sk, Gen, rnd, m = (_aligned(x) for x in (sk, Gen, rnd, m))
    n, ng = len(sk), len(Gen)
    u, R = _aligned(np.full((n, 32), 0xA5, np.uint8)), _aligned(np.full((n, 64), 0xA5, np.uint8))
    PK = _aligned(np.full((n, 64), 0xA5, np.uint8)) if want_pk else None
    G_out = _aligned(np.full((ng, 64), 0xA5, np.uint8)) if want_gen else None
    st = np.full(n, 0xA5, np.uint8)
    rc = load().jjs_sign_vargen_host(int(fmt_code), 1, int(route), _p(sk), _p(Gen), ctypes.c_size_t(ng), _p(rnd), _p(m), ctypes.c_size_t(n),
                                     ctypes.c_size_t(lanes), _p(u), _p(R), _p(PK), _p(G_out), _p(st))
    assert rc == 0, rc
    return u, R, PK, G_out, st


def derive(fmt_code, sk, Gen, lanes=3, want_gen=True):
    """One derivation call.  Returns (PK, Gen_out, status), prefilled with 0xA5."""
    sk, Gen = _aligned(sk), _aligned(Gen)
    n, ng = len(sk), len(Gen)
    PK = _aligned(np.full((n, 64), 0xA5, np.uint8))
    G_out = _aligned(np.full((ng, 64), 0xA5, np.uint8)) if want_gen else None
    st = np.full(n, 0xA5, np.uint8)
    rc = load().jjs_sign_vargen_host(int(fmt_code), 0, 0, _p(sk), _p(Gen), ctypes.c_size_t(ng), None, None, ctypes.c_size_t(n),
                                     ctypes.c_size_t(lanes), None, None, _p(PK), _p(G_out), _p(st))
    assert rc == 0, rc
    return PK, G_out, st

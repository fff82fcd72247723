"""ctypes loader for tests/hostbuild/libjjs_msig_sign_hosttest.so: csrc/msig_sign.h and the product headers compiled for the CPU
(the recipe of msig_verify_hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib
from msig_verify_hostlib import _aligned, _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_sign_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_sign_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def sign(c, signer_row, sk, r, s, lanes=3):
    """One signing call on the transcripts of an msig_sign_cases.SCase.  Returns (z, sign_status), both prefilled with 0xA5."""
    offs = _aligned(c.offs32(), np.uint32)
    PK, R, S, m, sk, r, s = (_aligned(x) for x in (c.PK, c.R, c.S, c.m, sk, r, s))
    rows = _aligned(signer_row, np.uint32) if signer_row is not None else None
    k = len(sk)
    z, st = _aligned(np.full((k, 32), 0xA5, np.uint8)), np.full(k, 0xA5, np.uint8)
    rc = load().jjs_msig_sign_host(int(c.fmt == "ext"), _p(PK), _p(R), _p(S), _p(m), _p(offs), ctypes.c_size_t(c.B), ctypes.c_size_t(lanes),
                                   _p(rows), _p(sk), _p(r), _p(s), ctypes.c_size_t(k), _p(z), _p(st))
    assert rc == 0, rc
    return z, st


def round1(r, s):
    """sign_round_1 of every row.  Returns (R, S, bad), prefilled with 0xA5."""
    r, s = _aligned(r), _aligned(s)
    n = len(r)
    R, S, bad = _aligned(np.full((n, 64), 0xA5, np.uint8)), _aligned(np.full((n, 64), 0xA5, np.uint8)), np.full(n, 0xA5, np.uint8)
    assert load().jjs_msig_sign_host_round1(_p(r), _p(s), ctypes.c_size_t(n), _p(R), _p(S), _p(bad)) == 0
    return R, S, bad

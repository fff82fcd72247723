"""ctypes loader for tests/hostbuild/libjjs_msig_share_hosttest.so: csrc/msig_share.h and the product headers compiled for the CPU
(the recipe of msig_verify_hostlib.py)."""
import ctypes
import os

import numpy as np

import msig_share_cases as shc
from hostlib import build_hostlib
from msig_verify_hostlib import _aligned, _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_share_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_share_hosttest.so")
ROUTES = {"inline": 0, "group": 1, "keyset": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def verify_share(sc, fmt="affine", want_R=True, lanes=3):
    """One call on a msig_share_cases.ShareCase.  Returns (share_status, sig_R or None), prefilled with 0xA5."""
    cols, m = sc.columns(fmt)
    offs = _aligned(sc.case.offsets.astype(np.uint32), np.uint32)
    R, S, m = _aligned(cols["R"]), _aligned(cols["S"]), _aligned(m)
    keys, idx = None, None
    if sc.route == "inline":
        keys = _aligned(cols["PK"])
    elif sc.route == "group":
        keys = _aligned(sc.group_pk)
    else:
        keys, idx = _aligned(sc.keys), _aligned(sc.key_idx, np.uint32)
    n_keys = 0 if sc.route == "inline" else len(keys)
    qt, qs, z = sc.queries()
    qt, qs, z = _aligned(qt, np.uint32), _aligned(qs, np.uint32), _aligned(z)
    st = np.full(sc.Q, 0xA5, np.uint8)
    sr = _aligned(np.full((sc.T, 64), 0xA5, np.uint8)) if want_R else None
    rc = load().jjs_msig_share_host(ROUTES[sc.route], shc.FORMAT_IDS[fmt], _p(keys), ctypes.c_size_t(n_keys), _p(idx), _p(R), _p(S), _p(m),
                                    _p(offs), ctypes.c_size_t(sc.T), ctypes.c_size_t(lanes), _p(qt), _p(qs), _p(z), ctypes.c_size_t(sc.Q),
                                    _p(st), _p(sr))
    assert rc == 0, rc
    return st, sr

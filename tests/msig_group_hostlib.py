"""ctypes loader for tests/hostbuild/libjjs_msig_group_hosttest.so: csrc/msig_group.h and the product headers compiled for the
CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_group_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_group_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _c(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def check_keys(PK) -> int:
    """What registration answers for this key vector before it builds anything: 0, or -1."""
    PK = _c(PK).reshape(-1, 64)
    return load().jjs_msig_group_host_check(_p(PK) if len(PK) else None, ctypes.c_size_t(len(PK)))


def combine(PK, z, R, S, m, by_participant=False):
    """Register PK and run one call.  Returns rc, (share_status, sig_u, sig_R, transcript_status), aggregate key."""
    PK, z, R, S, m = (_c(x) for x in (PK, z, R, S, m))
    n, B = len(PK), len(m)
    assert len(z) == len(R) == len(S) == n * B
    st, ts = np.full(n * B, 0xA5, np.uint8), np.full(B, 0xA5, np.uint8)
    su, sr, agg = np.full((B, 32), 0xA5, np.uint8), np.full((B, 64), 0xA5, np.uint8), np.zeros(64, np.uint8)
    rc = load().jjs_msig_group_host_combine(_p(PK), ctypes.c_size_t(n), _p(z), _p(R), _p(S), _p(m), ctypes.c_size_t(B), int(bool(by_participant)),
                                            _p(st), _p(ts), _p(su), _p(sr), _p(agg))
    return rc, (st, su, sr, ts), agg

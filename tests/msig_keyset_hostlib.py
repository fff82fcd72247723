"""ctypes loader for tests/hostbuild/libjjs_msig_keyset_hosttest.so: csrc/msig_keyset.h and the product headers compiled for the
CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_keyset_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_keyset_hosttest.so")
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


def combine(keys, key_idx, z, R, S, m, offsets):
    """Register `keys` and run one call.  Returns rc, key_status, (share_status, agg_pk, sig_u, sig_R, transcript_status)."""
    keys, z, R, S, m = (_c(x) for x in (keys, z, R, S, m))
    idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
    offs = np.ascontiguousarray(offsets, dtype=np.uint32)
    B, N = len(offs) - 1, len(z)
    assert len(idx) == len(R) == len(S) == N == int(offs[-1]) and len(m) == B
    ks = np.full(len(keys), 0xA5, np.uint8)
    st, ts = np.full(N, 0xA5, np.uint8), np.full(B, 0xA5, np.uint8)
    agg, su, sr = np.full((B, 64), 0xA5, np.uint8), np.full((B, 32), 0xA5, np.uint8), np.full((B, 64), 0xA5, np.uint8)
    rc = load().jjs_msig_keyset_host_combine(_p(keys), ctypes.c_size_t(len(keys)), _p(idx), _p(z), _p(R), _p(S), _p(m), _p(offs),
                                             ctypes.c_size_t(B), _p(ks), _p(st), _p(ts), _p(agg), _p(su), _p(sr))
    return rc, ks, (st, agg, su, sr, ts)

"""ctypes loader for tests/hostbuild/libjjs_msig_verify_hosttest.so: csrc/msig_verify.h and the product headers compiled for the
CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_verify_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_verify_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _aligned(a, dtype=np.uint8):
    """A C-contiguous copy at a 16-byte aligned address (the CPU build loads 16 bytes at a time)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    raw = np.empty(a.nbytes + 32, np.uint8)
    at = (-raw.ctypes.data) % 16
    out = raw[at:at + a.nbytes].view(dtype).reshape(a.shape)
    out[...] = a
    return out


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def run(rows, offsets, sig=None, keys=None, ext=False, lanes=3):
    """One call.  rows: the PK column (inline; (N, 96) with ext) or the index column (keys: the set to register).  sig None:
    aggregation alone, returns (agg_pk, vec_status); sig = (u, R, m): returns (status, tally, agg_pk).  Every output is
    prefilled with 0xA5."""
    offs = _aligned(offsets, np.uint32)
    B = len(offs) - 1
    rows = _aligned(rows, np.uint32 if keys is not None else np.uint8)
    assert len(rows) == int(offs[-1])
    hk = _aligned(keys) if keys is not None else None
    agg = _aligned(np.full((B, 64), 0xA5, np.uint8))
    vst, st, tally = np.full(B, 0xA5, np.uint8), np.full(B, 0xA5, np.uint8), np.full(4, 0xA5A5A5A5, np.uint64)
    u = R = m = None
    if sig is not None:
        u, R, m = (_aligned(x) for x in sig)
        assert len(u) == len(R) == len(m) == B and R.shape[1] == (96 if ext else 64)
    rc = load().jjs_msig_verify_host(_p(hk), ctypes.c_size_t(len(hk) if hk is not None else 0), _p(rows), int(bool(ext)), _p(offs),
                                     ctypes.c_size_t(B), ctypes.c_size_t(lanes), _p(u), _p(R), _p(m), _p(agg),
                                     _p(vst) if sig is None else None, _p(st) if sig is not None else None,
                                     _p(tally) if sig is not None else None)
    assert rc == 0, rc
    return (agg, vst) if sig is None else (st, tally, agg)

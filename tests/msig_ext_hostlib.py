"""ctypes loader for tests/hostbuild/libjjs_msig_ext_hosttest.so: normalize_lane in poison mode in front of the CPU build of the
multisignature passes and of the signer groups (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_ext_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_ext_hosttest.so")
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


def normalize(ext_arrays, lanes=1, poison=True):
    """(n, 96) columns -> (n, 64) columns, one item per row with len(ext_arrays) sources, run as `lanes` lanes; and the flags
    that the mode without poison writes."""
    ext = [_c(a) for a in ext_arrays]
    n, k = len(ext[0]), len(ext)
    outs = [np.full((n, 64), 0x5A, np.uint8) for _ in ext]
    bad = np.zeros(n, np.uint8)
    PP = ctypes.c_void_p * k
    load().jjs_msig_ext_host_normalize(PP(*[a.ctypes.data for a in ext]), k, ctypes.c_size_t(n), ctypes.c_size_t(lanes), int(bool(poison)),
                                       PP(*[a.ctypes.data for a in outs]), _p(bad))
    return outs, bad


def check_keys(PK_ext) -> int:
    PK_ext = _c(PK_ext).reshape(-1, 96)
    return load().jjs_msig_ext_host_check(_p(PK_ext) if len(PK_ext) else None, ctypes.c_size_t(len(PK_ext)))


def combine(z, PK_ext, R_ext, S_ext, m, offsets, lanes=1):
    z, PK_ext, R_ext, S_ext, m = (_c(x) for x in (z, PK_ext, R_ext, S_ext, m))
    offs = np.ascontiguousarray(offsets, dtype=np.uint32)
    B, N = len(offs) - 1, len(z)
    status, ts = np.full(N, 0xA5, np.uint8), np.full(B, 0xA5, np.uint8)
    agg, su, sr = np.full((B, 64), 0xA5, np.uint8), np.full((B, 32), 0xA5, np.uint8), np.full((B, 64), 0xA5, np.uint8)
    rc = load().jjs_msig_ext_host_combine(_p(z), _p(PK_ext), _p(R_ext), _p(S_ext), _p(m), _p(offs), ctypes.c_size_t(B), ctypes.c_size_t(lanes),
                                          _p(status), _p(agg), _p(su), _p(sr), _p(ts))
    assert rc == 0
    return status, agg, su, sr, ts


def group_combine(PK_ext, z, R_ext, S_ext, m, lanes=1, by_participant=False):
    """Register the extended keys and run one call.  Returns rc, (share_status, sig_u, sig_R, transcript_status), aggregate key."""
    PK_ext, z, R_ext, S_ext, m = (_c(x) for x in (PK_ext, z, R_ext, S_ext, m))
    n, B = len(PK_ext), len(m)
    st, ts = np.full(n * B, 0xA5, np.uint8), np.full(B, 0xA5, np.uint8)
    su, sr, agg = np.full((B, 32), 0xA5, np.uint8), np.full((B, 64), 0xA5, np.uint8), np.zeros(64, np.uint8)
    rc = load().jjs_msig_ext_host_group_combine(_p(PK_ext), ctypes.c_size_t(n), _p(z), _p(R_ext), _p(S_ext), _p(m), ctypes.c_size_t(B),
                                                ctypes.c_size_t(lanes), int(bool(by_participant)), _p(st), _p(ts), _p(su), _p(sr), _p(agg))
    return rc, (st, su, sr, ts), agg

"""ctypes loader for tests/hostbuild/libjjs_msig_wire_hosttest.so: msig_decode_lane, the lane body of msig_decode_kernel, and
the key decoding of jjs_msig_group_create_wire, compiled for the CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_wire_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_wire_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _aligned(a):
    """A C-contiguous uint8 copy at a 16-byte aligned address (the CPU build loads 16 bytes at a time)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    raw = np.empty(a.nbytes + 32, np.uint8)
    at = (-raw.ctypes.data) % 16
    out = raw[at:at + a.nbytes].reshape(a.shape)
    out[...] = a
    return out


def decode(sources, lanes=1):
    """sources: a list of up to three (array, offset) -- rows of the array's width, the 32 bytes of the point at `offset` of a
    row ((n, 32) and 0 for a packed column, (n, 64) and 32 for the R half of u || R rows).  Returns the (n, 64) columns, one
    per source, prefilled with 0x5A."""
    arrs = [_aligned(a) for a, _ in sources]
    n, k = len(arrs[0]), len(arrs)
    assert all(len(a) == n for a in arrs)
    outs = [_aligned(np.full((n, 64), 0x5A, np.uint8)) for _ in arrs]
    PP, U = ctypes.c_void_p * k, ctypes.c_uint32 * k
    rc = load().jjs_msig_wire_host_decode(PP(*[a.ctypes.data for a in arrs]), U(*[a.shape[1] for a in arrs]), U(*[off for _, off in sources]),
                                          k, ctypes.c_size_t(n), ctypes.c_size_t(lanes), PP(*[a.ctypes.data for a in outs]))
    assert rc == 0
    return outs


def decode_keys(PK_w):
    """jjs_msig_group_create_wire's look at its keys: (rc, (n, 64) affine keys)."""
    PK_w = _aligned(np.asarray(PK_w, np.uint8).reshape(-1, 32))
    out = _aligned(np.zeros((len(PK_w), 64), np.uint8))
    rc = load().jjs_msig_wire_host_keys(PK_w.ctypes.data_as(ctypes.c_void_p) if len(PK_w) else None, ctypes.c_size_t(len(PK_w)),
                                        out.ctypes.data_as(ctypes.c_void_p))
    return rc, out

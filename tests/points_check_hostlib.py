"""ctypes loader for tests/hostbuild/libjjs_points_check_hosttest.so: csrc/points_check.h and the product headers compiled for
the CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "points_check_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_points_check_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        for f in ("jjs_pc_host_affine_point", "jjs_pc_host_ext_point", "jjs_pc_host_wire_point"):
            getattr(_lib, f).restype = ctypes.c_uint32
    return _lib


def aligned(shape, fill=0xA5):
    """A uint8 array on a 64-byte boundary (the product's loads are 16 bytes wide), filled with a byte no answer has."""
    size = int(np.prod(shape))
    raw = np.empty(size + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + size].reshape(shape)
    a[...] = fill
    return a


def _in(a):
    if a is None:
        return None
    b = aligned(a.shape)
    b[...] = a
    return b


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def check(kind, scheme, fmt, cols, want_outs):
    """The call on the CPU.  cols: the input columns (None where the format has none); want_outs: one bool per output.  Returns
    (status, tally[4], outs) with None for the outputs not asked for."""
    cols = [_in(c) for c in cols]
    n = len(cols[0])
    widths = [64, 64] if kind == "keys" else [32, 64, 64]
    outs = [aligned((n, w)) if want else None for w, want in zip(widths, want_outs)]
    status, tally = aligned((n,)), np.zeros(4, np.uint64)
    fn = load().jjs_pc_host_keys_check if kind == "keys" else load().jjs_pc_host_signatures_check
    rc = fn(scheme, fmt, *[_p(c) for c in cols], ctypes.c_size_t(n), _p(status), _p(tally), *[_p(a) for a in outs])
    assert rc == 0
    return status, tally, outs


def point(fmt, row):
    """(status, decoded row or None) of one point through the per-point function of its format."""
    row = _in(np.ascontiguousarray(row, np.uint8))
    if fmt == "affine":
        return load().jjs_pc_host_affine_point(_p(row)), None
    if fmt == "ext":
        return load().jjs_pc_host_ext_point(_p(row)), None
    out = aligned((64,))
    return load().jjs_pc_host_wire_point(_p(row), _p(out)), out

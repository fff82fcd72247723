"""ctypes loader for tests/hostbuild/libjjs_digest_hosttest.so: csrc/digest.h and the product headers compiled for the CPU (the
recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib
from points_check_hostlib import aligned

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "digest_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_digest_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        _lib.jjs_dg_host_blocks.restype = ctypes.c_uint32
        _lib.jjs_dg_host_order.restype = None
        _lib.jjs_dg_host_tag.restype = None
        _lib.jjs_dg_host_two256.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _in(a):
    b = aligned(a.shape)
    b[...] = a
    return b


def digest(case, flags=0, ordered=True, want_status=True):
    """The call on the CPU.  Returns (rc, out, status); the outputs are pre-filled with 0xA5."""
    n = case["n"]
    inp = _in(case["in"])
    out, status = aligned((n, 32)), aligned((n,)) if want_status else None
    offsets = None if case["offsets"] is None else np.ascontiguousarray(case["offsets"], np.uint32)
    rc = load().jjs_dg_host_digest(case["fmt"], flags, _p(inp), _p(offsets), ctypes.c_size_t(case["k"]), ctypes.c_size_t(n), _p(out), _p(status),
                                   1 if ordered else 0)
    return rc, out, status


def order(offsets):
    offsets = np.ascontiguousarray(offsets, np.uint32)
    out = np.full(len(offsets) - 1, 0xFFFFFFFF, np.uint32)
    load().jjs_dg_host_order(_p(offsets), ctypes.c_size_t(len(out)), _p(out))
    return out


def element(fmt, row):
    out = aligned((32,))
    bad = load().jjs_dg_host_element(fmt, _p(_in(np.ascontiguousarray(row, np.uint8))), _p(out))
    return bad, out


def tag(length):
    out = aligned((32,))
    load().jjs_dg_host_tag(ctypes.c_uint32(length), _p(out))
    return out


def two256():
    out = aligned((32,))
    load().jjs_dg_host_two256(_p(out))
    return out

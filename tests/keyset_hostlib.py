"""ctypes loader for tests/hostbuild/libjjs_keyset_hosttest.so: csrc/keyset.h and the product headers compiled for the CPU
(the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "keyset_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_keyset_hosttest.so")
SCHEMES = {"single": 0, "double": 1, "vargen": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def verify(scheme, keys, idx, u, R, Rp, m, positions=0):
    """keys: list of (n_keys, 64) affine columns; positions 0 = the large variant, else the latency variant's lanes per
    equation.  Returns (status per item, key_status per key)."""
    keys = [np.ascontiguousarray(k, dtype=np.uint8) for k in keys]
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    cols = [np.ascontiguousarray(c, dtype=np.uint8) if c is not None else None for c in (u, R, Rp, m)]
    n, nk = len(idx), len(keys[0])
    status, key_status = np.empty(n, np.uint8), np.empty(nk, np.uint8)
    rc = load().jjs_keyset_host_verify(SCHEMES[scheme], _p(keys[0]), _p(keys[1]) if len(keys) > 1 else None, ctypes.c_uint32(nk),
                                       _p(idx), *[_p(c) for c in cols], ctypes.c_size_t(n), positions, _p(status), _p(key_status))
    assert rc == 0
    return status, key_status

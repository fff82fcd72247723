"""ctypes loader for tests/hostbuild/libjjs_keyset_lookup_hosttest.so: csrc/keyset_lookup.h and the product headers compiled
for the CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "keyset_lookup_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_keyset_lookup_hosttest.so")
SCHEMES = {"single": 0, "double": 1, "vargen": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        _lib.jjs_kl_hash_affine.restype = ctypes.c_uint64
        _lib.jjs_kl_slot_count.restype = ctypes.c_uint32
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _c(a, dtype=np.uint8):
    return np.ascontiguousarray(a, dtype=dtype) if a is not None else None


def slot_count(n_keys):
    return load().jjs_kl_slot_count(ctypes.c_uint32(n_keys))


def hash_affine(row: bytes, seed: int) -> int:
    pts = [np.frombuffer(row[p:p + 64], np.uint8).copy() for p in range(0, len(row), 64)]
    return load().jjs_kl_hash_affine(ctypes.c_uint32(len(pts)), _p(pts[0]), _p(pts[1]) if len(pts) > 1 else None, ctypes.c_uint64(seed))


def find(keys, fmt, queries, bad=None, order=None, seed=0, slots=0):
    """keys, queries: lists of one or two columns (the second may be None).  Returns (idx per query, the table's slots, the
    on-curve byte per key)."""
    keys = [_c(k) for k in keys if k is not None]
    queries = [_c(q) for q in queries if q is not None]
    nk, n = len(keys[0]), len(queries[0])
    bad, order = _c(bad), _c(order, np.uint32)
    n_slots = slots or slot_count(nk)
    idx, slots_out, on_curve = np.empty(n, np.uint32), np.empty(n_slots, np.uint32), np.empty(nk, np.uint8)
    rc = load().jjs_kl_host_find(ctypes.c_uint32(len(keys)), _p(keys[0]), _p(keys[1]) if len(keys) > 1 else None, _p(bad), ctypes.c_uint32(nk),
                                 _p(order), ctypes.c_uint64(seed), ctypes.c_uint32(slots), fmt, _p(queries[0]),
                                 _p(queries[1]) if len(queries) > 1 else None, ctypes.c_size_t(n), _p(idx), _p(slots_out), _p(on_curve))
    assert rc == 0
    return idx, slots_out, on_curve


def verify_keys(scheme, keys, K, u, R, Rp, m, positions=0, seed=0):
    """keys: the set's affine columns; K: the items' key columns.  Returns (status, tally[4], idx)."""
    keys, K = [_c(k) for k in keys], [_c(k) for k in K]
    cols = [_c(c) for c in (u, R, Rp, m)]
    n, nk = len(K[0]), len(keys[0])
    status, tally, idx = np.empty(n, np.uint8), np.zeros(4, np.uint64), np.empty(n, np.uint32)
    rc = load().jjs_kl_host_verify_keys(SCHEMES[scheme], _p(keys[0]), _p(keys[1]) if len(keys) > 1 else None, ctypes.c_uint32(nk),
                                        ctypes.c_uint64(seed), _p(K[0]), _p(K[1]) if len(K) > 1 else None, *[_p(c) for c in cols],
                                        ctypes.c_size_t(n), positions, _p(status), _p(tally), _p(idx))
    assert rc == 0
    return status, tally, idx

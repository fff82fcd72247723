"""ctypes loader for tests/hostbuild/libjjs_keyset_verdict_hosttest.so: csrc/keyset_verdict.h and the product headers
compiled for the CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "keyset_verdict_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_keyset_verdict_hosttest.so")
SCHEMES = {"single": 0, "double": 1, "vargen": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def verify_all(scheme, keys, idx, b, seed=bytes(32), c=0, poison=False):
    """keys: list of (n_keys, 64) affine columns; b: a batch dict (its key columns are not read).  Returns a dict: verdict,
    total (the affine combined sum, 64 bytes), key_sums (point columns x n_keys x 32), key_status, z_bits."""
    keys = [np.ascontiguousarray(k, dtype=np.uint8) for k in keys]
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    cols = [np.ascontiguousarray(b[k], dtype=np.uint8) if b.get(k) is not None else None for k in ("u", "R", "Rp", "m")]
    n, nk = len(idx), len(keys[0])
    verdict, z_bits = ctypes.c_int(-1), ctypes.c_int(0)
    total, sums, key_status = np.zeros(64, np.uint8), np.zeros((len(keys), nk, 32), np.uint8), np.empty(nk, np.uint8)
    rc = load().jjs_ksv_host_verify_all(SCHEMES[scheme], _p(keys[0]), _p(keys[1]) if len(keys) > 1 else None, ctypes.c_uint32(nk),
                                        _p(idx), *[_p(x) for x in cols], ctypes.c_size_t(n), seed, c, int(poison),
                                        ctypes.byref(verdict), _p(total), _p(sums), _p(key_status), ctypes.byref(z_bits))
    assert rc == 0
    return {"verdict": verdict.value, "total": total, "key_sums": sums, "key_status": key_status, "z_bits": z_bits.value}


def key_sums(scheme, keys, idxs, cols, poison=True):
    """The run sums and key points alone, for several cases against one set: idxs[i] the key indices of case i, cols[i] its
    scalar columns (list of (n_i, 32), below r).  Returns (sums (cases, point columns, n_keys, 32), the affine sums of
    S_k * P_k (cases, 64))."""
    keys = [np.ascontiguousarray(k, dtype=np.uint8) for k in keys]
    ns = np.array([len(i) for i in idxs], np.uint64)
    idx = np.ascontiguousarray(np.concatenate(idxs), dtype=np.uint32)
    a = [np.ascontiguousarray(np.concatenate([c[ci] for c in cols]), dtype=np.uint8) for ci in range(len(keys))]
    assert all(x.shape == (len(idx), 32) for x in a)
    nk = len(keys[0])
    sums, point = np.zeros((len(ns), len(keys), nk, 32), np.uint8), np.zeros((len(ns), 64), np.uint8)
    rc = load().jjs_ksv_host_key_sums(SCHEMES[scheme], _p(keys[0]), _p(keys[1]) if len(keys) > 1 else None, ctypes.c_uint32(nk),
                                      ctypes.c_size_t(len(ns)), _p(ns), _p(idx), _p(a[0]), _p(a[1]) if len(a) > 1 else None, int(poison),
                                      _p(sums), _p(point))
    assert rc == 0
    return sums, point


def items(scheme, keys, idx, b, seed, c, grids):
    """The keyed item pass alone on the CPU build, as jjs_debug_keyset_items_dev copies it out on the device.  Returns a dict:
    scalars, a (one column per point column of the set), partial ({blocks: the partial sums of a grid of that many blocks}),
    fail, zu."""
    keys = [np.ascontiguousarray(k, dtype=np.uint8) for k in keys]
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    cols = [np.ascontiguousarray(b[k], dtype=np.uint8) if b.get(k) is not None else None for k in ("u", "R", "Rp", "m")]
    n, nk, n_eq = len(idx), len(keys[0]), 2 if scheme == "double" else 1
    scalars, partial, zu = np.zeros(n_eq * n * 32, np.uint8), np.zeros(sum(grids) * 64, np.uint8), np.zeros(64, np.uint8)
    g = np.array(grids, np.uint32)
    a = [np.zeros(n * 32, np.uint8) for _ in keys]
    fail = ctypes.c_uint32(7)
    rc = load().jjs_ksv_host_items(SCHEMES[scheme], _p(keys[0]), _p(keys[1]) if len(keys) > 1 else None, ctypes.c_uint32(nk), _p(idx),
                                   *[_p(x) for x in cols], ctypes.c_size_t(n), seed, c, _p(g), ctypes.c_size_t(len(g)), _p(scalars), _p(a[0]),
                                   _p(a[1]) if len(a) > 1 else None, _p(partial), ctypes.byref(fail), _p(zu))
    assert rc == 0
    ends = np.cumsum(g) * 64
    return {"scalars": scalars.tobytes(), "a": [x.tobytes() for x in a], "partial": {int(k): partial[e - 64 * int(k):e].tobytes() for k, e in zip(g, ends)},
            "fail": fail.value, "zu": zu.tobytes()}

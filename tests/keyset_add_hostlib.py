"""ctypes loader for tests/hostbuild/libjjs_keyset_add_hosttest.so: csrc/keyset_add.h and the product headers compiled for the
CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "keyset_add_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_keyset_add_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        _lib.jjs_kl_slot_count.restype = ctypes.c_uint32
        _lib.jjs_ka_host_scan.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _c(a, dtype=np.uint8):
    return np.ascontiguousarray(a, dtype=dtype) if a is not None else None


def _aligned(a):
    """A 16-byte aligned copy: the set's rows are read with 16-byte loads."""
    a = _c(a)
    buf = np.empty(a.size + 16, np.uint8)
    off = (-buf.ctypes.data) % 16
    out = buf[off:off + a.size].reshape(a.shape)
    out[...] = a
    return out


def add(set_cols, set_bad, fmt, cand_cols, unique, seed=0):
    """set_cols: the set's affine columns (the second may be None); cand_cols: the candidates' columns in `fmt` (0 affine, 1 ext,
    2 wire).  Returns a dict: idx, status, n_added, rows (per column, the set afterwards), flags (per column), slots (the lookup
    table after the add), fresh (the table of a fresh build), rebuilt."""
    sc = [_aligned(c) for c in set_cols if c is not None]
    cc = [_aligned(c) for c in cand_cols if c is not None]
    cols, n_old, n = len(sc), len(sc[0]), len(cc[0])
    room = n_old + n
    bad = _c(set_bad)
    idx, status = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rows, flags = np.zeros((cols, room, 64), np.uint8), np.zeros((cols, room), np.uint8)
    max_slots = load().jjs_kl_slot_count(ctypes.c_uint32(room))
    slots, fresh = np.empty(max_slots, np.uint32), np.empty(max_slots, np.uint32)
    n_added, rebuilt = ctypes.c_uint32(0), ctypes.c_int(0)
    rc = load().jjs_ka_host_add(ctypes.c_uint32(cols), int(fmt), 1 if unique else 0, _p(sc[0]), _p(sc[1]) if cols > 1 else None, _p(bad),
                                ctypes.c_uint32(n_old), _p(cc[0]), _p(cc[1]) if len(cc) > 1 else None, ctypes.c_uint32(n), ctypes.c_uint64(seed),
                                _p(idx), _p(status), ctypes.byref(n_added), _p(rows), _p(flags), _p(slots), _p(fresh), ctypes.byref(rebuilt))
    assert rc == 0, rc
    n_new = n_old + n_added.value
    s = load().jjs_kl_slot_count(ctypes.c_uint32(n_new))
    return {"idx": idx, "status": status, "n_added": n_added.value, "rows": [rows[c, :n_new] for c in range(cols)],
            "flags": [flags[c, :n_new] for c in range(cols)], "slots": slots[:s], "fresh": fresh[:s], "rebuilt": bool(rebuilt.value)}


def scan(counts):
    """The exclusive scan of the block counts as keyset_add_scan_kernel leaves it: (scan, total)."""
    sums = np.zeros(len(counts) + 1, np.uint32)
    sums[:-1] = counts
    load().jjs_ka_host_scan(_p(sums), ctypes.c_uint32(len(counts)))
    return sums[:-1], int(sums[-1])

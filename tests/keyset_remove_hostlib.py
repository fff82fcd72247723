"""ctypes loader for tests/hostbuild/libjjs_keyset_remove_hosttest.so: csrc/keyset_remove.h and the product headers compiled for
the CPU (the recipe of hostlib.py).  A `Session` is one set, as a device copy holds it."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "keyset_remove_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_keyset_remove_hosttest.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        _lib.jjs_kr_new.restype = ctypes.c_void_p
        for name in ("jjs_kr_keys", "jjs_kr_slot_count", "jjs_kr_table_units", "jjs_kr_pattern"):
            getattr(_lib, name).restype = ctypes.c_uint32
        _lib.jjs_kr_free.restype = _lib.jjs_kr_find.restype = _lib.jjs_kr_state.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _cols(rows, cols):
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 64 * cols)
    return [np.ascontiguousarray(a[:, 64 * c:64 * c + 64]) for c in range(cols)] + [None] * (2 - cols)


def _u32(x):
    return ctypes.c_uint32(int(x))


class Session:
    def __init__(self, rows, flags, cols, cap=None, seed=0, tables=False):
        """rows: the keys (64 * cols bytes each); flags: the KT_KEY_* byte per key (every point column gets it)."""
        self.cols, self.lib = cols, load()
        r = _cols(rows, cols)
        f = np.ascontiguousarray(flags, np.uint8)
        self.h = ctypes.c_void_p(self.lib.jjs_kr_new(_u32(cols), _p(r[0]), _p(r[1]), _p(f), _p(f), _u32(len(rows)), _u32(cap or len(rows)),
                                                     ctypes.c_uint64(seed), int(tables)))
        assert self.h

    def close(self):
        if self.h:
            self.lib.jjs_kr_free(self.h)
            self.h = None

    @property
    def n(self):
        return self.lib.jjs_kr_keys(self.h)

    def remove(self, idx, backwards=False):
        """(result, [distinct removed, those that were valid])."""
        idx = np.ascontiguousarray(idx, np.uint32)
        res, counts = np.full(len(idx), 0xEE, np.uint8), np.zeros(2, np.uint32)
        assert self.lib.jjs_kr_remove(self.h, _p(idx), _u32(len(idx)), _p(res), _p(counts), int(backwards)) == 0
        return res, counts.tolist()

    def find(self, rows):
        q = _cols(rows, self.cols)
        out = np.empty(len(rows), np.uint32)
        self.lib.jjs_kr_find(self.h, _p(q[0]), _p(q[1]), _u32(len(rows)), _p(out))
        return out

    def state(self):
        """(flags [cols][n], slots, rows as a list of bytes)."""
        n = self.n
        flags, slots = np.empty((self.cols, n), np.uint8), np.empty(self.lib.jjs_kr_slot_count(self.h), np.uint32)
        rows = np.empty((self.cols, n, 64), np.uint8)
        self.lib.jjs_kr_state(self.h, _p(flags), _p(slots), _p(rows))
        return flags, slots, [b"".join(rows[c, i].tobytes() for c in range(self.cols)) for i in range(n)]

    def add(self, rows, flags, unique):
        r = _cols(rows, self.cols)
        f = np.ascontiguousarray(flags, np.uint8)
        idx = np.empty(len(rows), np.uint32)
        assert self.lib.jjs_kr_add(self.h, _p(r[0]), _p(r[1]), _p(f), _p(f), _u32(len(rows)), int(unique), _p(idx)) == 0
        return idx

    def compact(self, backwards=False):
        """(the map, the new key count)."""
        m = np.full(self.n, 0xEEEEEEEE, np.uint32)
        n_new = self.lib.jjs_kr_compact(self.h, _p(m), int(backwards))
        return m, n_new

    def table(self, col, key):
        out = np.empty(4 * self.lib.jjs_kr_table_units(), np.uint32)
        assert self.lib.jjs_kr_table(self.h, _u32(col), _u32(key), _p(out)) == 0
        return out


def pattern_table(col, key):
    """The words the harness gave key `key`'s table in column `col` when the session was made."""
    units = load().jjs_kr_table_units()
    u = np.repeat(np.arange(units, dtype=np.uint64), 4)
    w = np.tile(np.arange(4, dtype=np.uint64), units)
    v = ((key * 2654435761) & 0xFFFFFFFF) ^ ((col * 0x9E3779B9) & 0xFFFFFFFF) ^ ((u * 40503 + w * 7 + (u >> np.uint64(7))) & 0xFFFFFFFF)
    out = v.astype(np.uint32)
    assert int(out[5]) == load().jjs_kr_pattern(_u32(col), _u32(key), _u32(1), _u32(1))
    return out

"""ctypes loader for tests/hostbuild/libjjs_key_memo_hosttest.so: the key-table path with the memo of the slot's last call
(csrc/key_tables.h step 5) compiled for the CPU (the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "key_memo_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_key_memo_hosttest.so")
SCHEMES = {"single": 0, "double": 1, "vargen": 2}
KEY_COLUMNS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        _lib.jjs_memo_host_new.restype = ctypes.c_void_p
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Slot:
    """A call slot of the CPU build: its pool and its memo outlive the calls."""

    def __init__(self, cap):
        self.h = ctypes.c_void_p(load().jjs_memo_host_new(ctypes.c_uint32(cap)))

    def close(self):
        if self.h:
            load().jjs_memo_host_free(self.h)
            self.h = None

    def new_pool(self):
        """What a reallocated or trimmed pool looks like to the next call."""
        load().jjs_memo_host_new_pool(self.h)

    def call(self, scheme, b, window, off=False):
        """Returns (statuses, hits per column, built keys per column); window 0 = the batch turns the tables down."""
        cols = {k: np.ascontiguousarray(v, dtype=np.uint8) for k, v in b.items()}
        n = len(cols["u"])
        k2 = {"single": None, "double": "PKp", "vargen": "Gen"}[scheme]
        status = np.full(n, 255, np.uint8)
        counts = np.zeros(4, np.uint32)
        rc = load().jjs_memo_host_call(self.h, SCHEMES[scheme], _p(cols["u"]), _p(cols["R"]), _p(cols.get("Rp")), _p(cols["PK"]),
                                       _p(cols[k2]) if k2 else None, _p(cols["m"]), ctypes.c_size_t(n), int(window), int(bool(off)),
                                       _p(status), _p(counts))
        assert rc == 0, rc
        nc = len(KEY_COLUMNS[scheme])
        return status, counts[:nc].tolist(), counts[2:2 + nc].tolist()

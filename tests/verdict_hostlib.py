"""ctypes loader for tests/hostbuild/libjjs_verdict_hosttest.so: csrc/batch_verdict.h and csrc/msm.h compiled for the CPU
(the recipe of hostlib.py)."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "verdict_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_verdict_hosttest.so")
SCHEMES = {"single": 0, "double": 1, "vargen": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    out = ctypes.create_string_buffer(64)
    assert load().jjs_vh_chacha20_block(key, ctypes.c_uint32(counter), nonce, out) == 0
    return out.raw


def msm(points, scalars, neg=None, c=0, short=False, stages=False):
    """points: (N, 64) affine; scalars: (N, 32) below 2^252 (short: within the weights' bits); neg: N flags (the term is -P).
    Returns the affine sum (64 bytes); with stages a dict: total, off (W * B + 1), order (off[-1] entries), win (W, 64)."""
    points = np.ascontiguousarray(points, np.uint8)
    scalars = np.ascontiguousarray(scalars, np.uint8)
    neg = np.ascontiguousarray(np.zeros(len(points), np.uint8) if neg is None else neg, np.uint8)
    out = np.zeros(64, np.uint8)
    off = order = win = None
    if stages:
        assert c
        W = (129 if short else 253) // c + ((129 if short else 253) % c != 0)
        off, order, win = np.zeros((W << (c - 1)) + 1, np.uint32), np.zeros(len(points) * W, np.uint32), np.zeros((W, 64), np.uint8)
    assert load().jjs_vh_msm(_p(points), _p(scalars), _p(neg), ctypes.c_size_t(len(points)), c, int(short), _p(out), _p(off), _p(order),
                             _p(win)) == 0
    return {"total": out, "off": off, "order": order[:off[-1]], "win": win} if stages else out


def verify_all(scheme, b, seed=bytes(32), c=0):
    """The batch verdict of the CPU build for a batch dict (helpers.make_batch): 1 or 0."""
    cols = {k: np.ascontiguousarray(v, np.uint8) for k, v in b.items()}
    second = cols.get("PKp") if scheme == "double" else cols.get("Gen")
    verdict = ctypes.c_int(-1)
    rc = load().jjs_vh_verify_all(SCHEMES[scheme], _p(cols["u"]), _p(cols["R"]), _p(cols.get("Rp")), _p(cols["PK"]), _p(second),
                                  _p(cols["m"]), ctypes.c_size_t(len(cols["u"])), seed, c, ctypes.byref(verdict))
    assert rc == 0
    return verdict.value


def verdict_items(scheme, cols, seed, c, grids):
    """The item pass of the batch verdict on the CPU build, as jjs_debug_verdict_items_dev copies it out on the device.  cols:
    the six column slots (verdict_item_cases.batch_columns); grids: block counts.  Returns a dict: scalars, partial ({blocks: the
    partial sums of a grid of that many blocks}), fail, zu."""
    cols = [np.ascontiguousarray(x, np.uint8) if x is not None else None for x in cols]
    n = len(cols[0])
    u, r, rp, pk, second, m = (cols[0], cols[1], cols[2], cols[3], cols[4], cols[5]) if scheme == "double" else \
        (cols[0], cols[1], None, cols[2], None, cols[3]) if scheme == "single" else (cols[0], cols[1], None, cols[2], cols[3], cols[4])
    kinds = {"single": 2, "double": 4, "vargen": 3}[scheme]
    scalars, partial, zu = np.zeros(kinds * n * 32, np.uint8), np.zeros(sum(grids) * 64, np.uint8), np.zeros(64, np.uint8)
    fail = ctypes.c_uint32(7)
    g = np.array(grids, np.uint32)
    rc = load().jjs_vh_verdict_items(SCHEMES[scheme], _p(u), _p(r), _p(rp), _p(pk), _p(second), _p(m), ctypes.c_size_t(n), seed, c,
                                     _p(g), ctypes.c_size_t(len(g)), _p(scalars), _p(partial), ctypes.byref(fail), _p(zu))
    assert rc == 0
    ends = np.cumsum(g) * 64
    return {"scalars": scalars.tobytes(), "partial": {int(k): partial[e - 64 * int(k):e].tobytes() for k, e in zip(g, ends)}, "fail": fail.value,
            "zu": zu.tobytes()}

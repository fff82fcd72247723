"""ctypes loader for tests/hostbuild/libjjs_keyset_hosttest.so: csrc/keyset.h and the product headers compiled for the CPU
(the recipe of hostlib.py)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostbuild", "keyset_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_keyset_hosttest.so")
CSRC = os.path.join(ROOT, "jubjub_schnorr_amd", "csrc")
SCHEMES = {"single": 0, "double": 1, "vargen": 2}
_lib = None


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [SRC, os.path.join(HERE, "hostbuild", "host_harness.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    return any(os.path.getmtime(d) > t for d in deps)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if _stale():
        san = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if os.environ.get("JJS_HOST_SANITIZE") else ["-O2"]
        subprocess.check_call(["g++", *san, "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                               "-I" + CSRC, "-o", LIB, SRC])
    _lib = ctypes.CDLL(LIB)
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

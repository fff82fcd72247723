"""ctypes loader for tests/hostbuild/libjjs_msig_scratch_hosttest.so: csrc/msig_scratch.h compiled for the CPU."""
import ctypes
import os

import numpy as np

from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "msig_scratch_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_msig_scratch_hosttest.so")
_lib = None

DIMS = ["rows", "transcripts", "ext_rows", "ks_rows", "ks_transcripts", "sign_rows", "sign_transcripts", "share_queries", "share_transcripts"]
# The regions in the order the harness reports them: name, the dimension without which the region is null, alignment.
REGIONS = [("tr_of", "rows", 4), ("d_words", "rows", 4), ("dpk", "rows", 4), ("e_pt", "rows", 4),
           ("a_words", "transcripts", 4), ("c_words", "transcripts", 4), ("offsets", "transcripts", 4), ("long_tags", "transcripts", 4),
           ("norm0", "ext_rows", 64), ("norm1", "ext_rows", 64), ("norm2", "ext_rows", 64), ("prefix", "ext_rows", 4),
           ("ks_pk", "ks_rows", 64), ("ks_row_key", "ks_rows", 4), ("ks_refused", "ks_rows", 4),
           ("pk_repeats", "sign_rows", 4), ("bad_enc", "sign_rows", 4), ("dup_nonce", "sign_rows", 4), ("sign_agg", "sign_rows", 64), ("sign_rsa", "sign_rows", 64),
           ("share_pt", "share_queries", 4), ("share_bad", "share_queries", 4), ("share_agg", "share_queries", 64), ("share_rsa", "share_queries", 64)]


def load():
    global _lib
    if _lib is None:
        _lib = build_hostlib(SRC, LIB)
        _lib.jjs_msig_scratch_layout.restype = ctypes.c_uint64
    return _lib


def _v(caps):
    return np.array([caps[d] for d in DIMS], np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ext_words():
    return load().jjs_msig_scratch_ext_words()


def layout(base, caps):
    """The walk at address `base` over capacities `caps` (a dict over DIMS): ({region: address or 0}, bytes, sign_flag_words)."""
    regions, words = np.zeros(len(REGIONS), np.uint64), ctypes.c_uint64(0)
    nbytes = load().jjs_msig_scratch_layout(ctypes.c_uint64(base), _p(_v(caps)), _p(regions), ctypes.byref(words))
    return {name: int(a) for (name, _, _), a in zip(REGIONS, regions)}, int(nbytes), int(words.value)


def grown(held, need):
    out = np.zeros(len(DIMS), np.uint64)
    load().jjs_msig_scratch_grown(_p(_v(held)), _p(_v(need)), _p(out))
    return dict(zip(DIMS, (int(x) for x in out)))

"""The verifier's multisignature calls in the C ABI and its Python mirror: the eight symbols exported and bound with the argument
counts of include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the mirror's signatures.  No GPU: the library is
loaded, never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = {"jjs_multisig_aggregate_pk_dev": 7, "jjs_multisig_aggregate_pk": 6, "jjs_multisig_aggregate_pk_keyset_dev": 7,
           "jjs_multisig_aggregate_pk_keyset": 6, "jjs_multisig_verify_dev": 11, "jjs_multisig_verify": 10,
           "jjs_multisig_verify_keyset_dev": 12, "jjs_multisig_verify_keyset": 11}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_eight_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    raw = ctypes.CDLL(LIB)
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for name, argc in SYMBOLS.items():
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES and getattr(lib, name).argtypes == _ffi.SIGNATURES[name], name
        assert len(_ffi.SIGNATURES[name]) == argc, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl and len(decl.group(1).split(",")) == argc, (name, "the header's argument count")
    assert lib.jjs_abi_version() == 5, "the additions are additive"
    prof = open(os.path.join(ROOT, "include", "jjs_gpu_profiling.h")).read()
    assert "multisig_verify" not in prof and "aggregate_pk" not in prof


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for fmt in (0, 1, 2):
        assert lib.jjs_multisig_aggregate_pk_dev(fmt, None, None, 1, None, None, None) == -4
        assert lib.jjs_multisig_aggregate_pk(fmt, None, None, 1, None, None) == -4
        assert lib.jjs_multisig_verify_dev(fmt, *[None] * 5, 1, *[None] * 4) == -4
        assert lib.jjs_multisig_verify(fmt, *[None] * 5, 1, *[None] * 3) == -4
        assert lib.jjs_multisig_verify_keyset_dev(1, fmt, *[None] * 5, 1, *[None] * 4) == -4
        assert lib.jjs_multisig_verify_keyset(1, fmt, *[None] * 5, 1, *[None] * 3) == -4
    assert lib.jjs_multisig_aggregate_pk_keyset_dev(1, None, None, 1, None, None, None) == -4
    assert lib.jjs_multisig_aggregate_pk_keyset(1, None, None, 1, None, None) == -4
    assert lib.jjs_multisig_verify_dev(0, *[None] * 5, 0, *[None] * 4) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_mirror_and_the_header():
    from jubjub_schnorr_amd.api import Engine, KeySet
    p = inspect.signature(Engine.multisig_aggregate_pk).parameters
    assert list(p)[1:] == ["PK", "offsets", "fmt"] and p["fmt"].default == "affine"
    p = inspect.signature(Engine.multisig_verify).parameters
    assert list(p)[1:] == ["PK", "offsets", "u", "R", "m", "fmt", "want_status"] and p["fmt"].default == "affine" and p["want_status"].default is True
    assert list(inspect.signature(KeySet.multisig_aggregate_pk).parameters)[1:] == ["key_idx", "offsets"]
    p = inspect.signature(KeySet.multisig_verify).parameters
    assert list(p)[1:] == ["key_idx", "offsets", "u", "R", "m", "fmt", "want_status"] and p["fmt"].default == "affine"
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for needle in ("UNUSABLE", "An EMPTY vector is usable", "NOT that of jjs_verify_single_ext", "on the curve"):
        assert needle in text, needle
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    for needle in ("aggregate_pk", "jjs_multisig_verify_keyset", "jjs_multisig_aggregate_pk_keyset", "multisig_verify"):
        assert needle in hpp, needle

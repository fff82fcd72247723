"""The signer's multisignature calls in the C ABI and its Python mirror: the three symbols exported and bound with the argument
counts of include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the new status constant, the mirror's signatures and
what the header must say.  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = {"jjs_multisig_round1_dev": 7, "jjs_multisig_sign_dev": 15, "jjs_multisig_sign": 14}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_three_symbols_are_exported_and_bound(lib):
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
    assert re.search(r"#define JJS_STATUS_DUPLICATED_NONCE 7\b", text)
    assert re.search(r"#define JJS_STATUS_INVALID_TRANSCRIPT 5\b", text)


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    assert lib.jjs_multisig_round1_dev(None, None, 1, None, None, None, None) == -4
    assert lib.jjs_multisig_round1_dev(None, None, 0, None, None, None, None) == -4
    for fmt in (0, 1, 2):
        for k in (0, 1):
            assert lib.jjs_multisig_sign_dev(fmt, *[None] * 5, k, *[None] * 4, k, None, None, None) == -4
            assert lib.jjs_multisig_sign(fmt, *[None] * 5, k, *[None] * 4, k, None, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_mirror_and_the_header():
    from jubjub_schnorr_amd.api import Engine
    assert list(inspect.signature(Engine.multisig_sign_round1).parameters)[1:] == ["r", "s"]
    p = inspect.signature(Engine.multisig_sign_round2).parameters
    assert list(p)[1:] == ["PK", "R", "S", "m", "offsets", "sk", "r", "s", "signer_row", "fmt"]
    assert p["signer_row"].default is None and p["fmt"].default == "affine"
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for needle in ("NOT constant time", "MultisigNonce", "the caller's error", "Row search", "TOLD the row", "profiles/r14_msig_sign.jsonl"):
        assert needle in text, needle
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    for needle in ("sign_round_1", "sign_round_2", "InvalidMultisigTranscript", "DuplicatedNonce", "jjs_multisig_sign"):
        assert needle in hpp, needle

"""verify_share on its own in the C ABI and its mirrors: the six symbols exported and bound with the argument counts of
include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the mirrors' signatures and what the two headers must say.
No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = {"jjs_multisig_verify_share_dev": 14, "jjs_multisig_verify_share": 13, "jjs_msig_group_verify_share_dev": 13,
           "jjs_msig_group_verify_share": 12, "jjs_multisig_verify_share_keyset_dev": 15, "jjs_multisig_verify_share_keyset": 14}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_six_symbols_are_exported_and_bound(lib):
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
    assert re.search(r"#define JJS_STATUS_INVALID_TRANSCRIPT 5\b", text)


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for fmt in (0, 1, 2, 7):
        for B in (0, 1):
            for Q in (0, 1):
                assert lib.jjs_multisig_verify_share_dev(fmt, *[None] * 5, B, *[None] * 3, Q, None, None, None) == -4
                assert lib.jjs_multisig_verify_share(fmt, *[None] * 5, B, *[None] * 3, Q, None, None) == -4
                assert lib.jjs_msig_group_verify_share_dev(1, fmt, *[None] * 3, B, *[None] * 3, Q, None, None, None) == -4
                assert lib.jjs_msig_group_verify_share(1, fmt, *[None] * 3, B, *[None] * 3, Q, None, None) == -4
                assert lib.jjs_multisig_verify_share_keyset_dev(1, fmt, *[None] * 5, B, *[None] * 3, Q, None, None, None) == -4
                assert lib.jjs_multisig_verify_share_keyset(1, fmt, *[None] * 5, B, *[None] * 3, Q, None, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_mirrors_and_the_headers():
    from jubjub_schnorr_amd.api import Engine, KeySet, SignerGroup
    queries = ["share_transcript", "share_slot", "z", "fmt", "want_R"]
    p = inspect.signature(Engine.multisig_verify_share).parameters
    assert list(p)[1:] == ["PK", "R", "S", "m", "offsets"] + queries
    assert p["fmt"].default == "affine" and p["want_R"].default is False
    p = inspect.signature(SignerGroup.verify_share).parameters
    assert list(p)[1:] == ["R", "S", "m"] + queries and p["fmt"].default == "affine" and p["want_R"].default is False
    p = inspect.signature(KeySet.multisig_verify_share).parameters
    assert list(p)[1:] == ["key_idx", "R", "S", "m", "offsets"] + queries and p["fmt"].default == "affine" and p["want_R"].default is False
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for needle in ("verify_share", "participant_index", "share_transcript", "share_slot", "profiles/r21_msig_share.jsonl"):
        assert needle in text, needle
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    for needle in ("verify_share", "participant_index", "InvalidMultisigShare", "profiles/r21_msig_share.jsonl", "verify_share_batch", "jjs_multisig_verify_share",
                   "jjs_msig_group_verify_share", "jjs_multisig_verify_share_keyset"):
        assert needle in hpp, needle

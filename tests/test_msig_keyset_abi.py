"""The multisignature call against a registered key set in the C ABI and its Python mirror: exported, bound with the argument
counts of include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged.  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = {"jjs_multisig_combine_keyset_dev": 15, "jjs_multisig_combine_keyset": 14}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_two_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    raw = ctypes.CDLL(LIB)
    for name, argc in SYMBOLS.items():
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES and getattr(lib, name).argtypes == _ffi.SIGNATURES[name], name
        assert len(_ffi.SIGNATURES[name]) == argc, name
    # the inline call's arguments with the handle and the format in front and the indices in place of PK
    assert _ffi.SIGNATURES["jjs_multisig_combine_keyset_dev"][2:] == _ffi.SIGNATURES["jjs_multisig_combine_dev"]
    assert _ffi.SIGNATURES["jjs_multisig_combine_keyset"][1:] == _ffi.SIGNATURES["jjs_multisig_combine"]
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for fmt in (0, 1, 2):
        assert lib.jjs_multisig_combine_keyset_dev(1, fmt, *[None] * 6, 1, *[None] * 6) == -4
        assert lib.jjs_multisig_combine_keyset(1, fmt, *[None] * 6, 1, *[None] * 5) == -4
    assert lib.jjs_multisig_combine_keyset_dev(0, 0, *[None] * 6, 0, *[None] * 6) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_mirror_and_the_header():
    from jubjub_schnorr_amd.api import KeySet
    p = inspect.signature(KeySet.multisig_combine).parameters
    assert list(p)[1:] == ["key_idx", "z", "R", "S", "m", "offsets", "fmt"] and p["fmt"].default == "affine"
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(jjs_keyset ks, int format, " in text, name
    assert "DIFFERENCE FROM THE REFERENCE" in text and "USABLE" in text
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    assert "multisig_combine" in hpp and "jjs_multisig_combine_keyset" in hpp

"""Var-generator signing and key derivation with the generator as a point in the C ABI and its Python mirror: the five symbols
exported and bound with the argument counts of include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the mirror's
signatures and what the header must say.  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = {"jjs_public_keys_vargen_dev": 9, "jjs_sign_vargen_pt_dev": 13, "jjs_public_keys_vargen": 8, "jjs_sign_vargen_pt": 12,
           "jjs_debug_sign_limits": 1}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_five_symbols_are_exported_and_bound(lib):
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


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for fmt in (0, 1, 2):
        for n in (0, 1):
            assert lib.jjs_public_keys_vargen_dev(fmt, None, None, n, n, None, None, None, None) == -4
            assert lib.jjs_sign_vargen_pt_dev(fmt, None, None, n, None, None, n, None, None, None, None, None, None) == -4
            assert lib.jjs_public_keys_vargen(fmt, None, None, n, n, None, None, None) == -4
            assert lib.jjs_sign_vargen_pt(fmt, None, None, n, None, None, n, None, None, None, None, None) == -4
    assert lib.jjs_sign_vargen_pt(7, None, None, 3, None, None, 9, None, None, None, None, None) == -4, "before any argument is looked at"
    assert lib.jjs_debug_sign_limits(None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_mirror_and_the_header():
    from jubjub_schnorr_amd import SecretKeyVarGen
    from jubjub_schnorr_amd.api import Engine
    p = inspect.signature(Engine.public_keys_vargen).parameters
    assert list(p)[1:] == ["sk", "Gen", "fmt"] and p["fmt"].default == "affine"
    p = inspect.signature(Engine.sign_vargen_pt).parameters
    assert list(p)[1:] == ["sk", "Gen", "rnd", "m", "fmt"] and p["fmt"].default == "affine"
    for member in ("new", "from_bytes", "to_bytes", "public_key", "sign", "sign_batch"):
        assert callable(getattr(SecretKeyVarGen, member)), member
    # the byte forms need no engine: the split of sk || generator is host slicing, the compression of `new`'s generator too
    raw = bytes(range(64))
    k = SecretKeyVarGen.from_bytes(raw)
    assert (k.sk, k.generator, k.fmt) == (raw[:32], raw[32:], "wire") and k.to_bytes() == raw
    a = SecretKeyVarGen.new(raw[:32], bytes([3]) + bytes(31) + bytes(range(32)))
    assert a.fmt == "affine" and a.to_bytes() == raw[:32] + bytes(range(31)) + bytes([31 | 0x80])
    with pytest.raises(ValueError):
        SecretKeyVarGen.from_bytes(raw[:63])
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for needle in ("NOT constant time", "profiles/r17_sign_vargen_pt.jsonl", "n_gen is n (one generator per item) or 1", "any other value gives -1",
                   "SecretKeyVarGen", "not on the curve", "status-3 item is zero bytes"):
        assert needle in text, needle
    for name in ("sign_vargen.h", "sign_vargen_calls.h"):
        assert "NOT constant time" in open(os.path.join(ROOT, "jubjub_schnorr_amd", "csrc", name)).read(), name
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    for needle in ("class SecretKeyVarGen", "with_variable_generator", "jjs_sign_vargen_pt", "jjs_public_keys_vargen", "NOT constant time"):
        assert needle in hpp, needle

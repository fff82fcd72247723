"""Signing and key derivation with a SecretKey (single and double scheme) in the C ABI and its Python mirror: the five symbols
exported and bound with the argument counts of include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the mirror's
signatures, SecretKey.from_bytes without a device, and what the header must say.  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = {"jjs_sign_fixed_dev": 15, "jjs_sign_fixed": 14, "jjs_public_keys_fixed_dev": 8, "jjs_public_keys_fixed": 7,
           "jjs_debug_sign_fixed_limits": 1}
R_ORDER = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7


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
    for scheme in (0, 1):
        for n in (0, 1):
            assert lib.jjs_sign_fixed_dev(scheme, None, n, None, None, n, None, None, None, None, None, None, None, None, None) == -4
            assert lib.jjs_sign_fixed(scheme, None, n, None, None, n, None, None, None, None, None, None, None, None) == -4
            assert lib.jjs_public_keys_fixed_dev(scheme, None, n, None, None, None, None, None) == -4
            assert lib.jjs_public_keys_fixed(scheme, None, n, None, None, None, None) == -4
    assert lib.jjs_sign_fixed(7, None, 3, None, None, 9, None, None, None, None, None, None, None, None) == -4, "before any argument is looked at"
    assert lib.jjs_debug_sign_fixed_limits(None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_secret_key_from_bytes_without_a_device():
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import Malformed, SecretKey
    assert "SecretKey" in dir(jjs)
    with pytest.raises(Malformed):
        SecretKey.from_bytes(R_ORDER.to_bytes(32, "little"))
    with pytest.raises(Malformed):
        SecretKey.from_bytes(b"\xff" * 32)
    with pytest.raises(ValueError):
        SecretKey.from_bytes(bytes(31))
    for v in (0, 1, R_ORDER - 1):
        raw = v.to_bytes(32, "little")
        k = SecretKey.from_bytes(raw)
        assert k.to_bytes() == raw and k.sk == raw
    g = bytes(range(64))
    vg = SecretKey.from_bytes(bytes(32)).with_variable_generator(g)
    assert isinstance(vg, jjs.SecretKeyVarGen) and (vg.sk, vg.generator, vg.fmt) == (bytes(32), g, "affine")


def test_the_mirror_and_the_header():
    from jubjub_schnorr_amd import SecretKey
    from jubjub_schnorr_amd.api import Engine
    p = inspect.signature(Engine.sign_fixed).parameters
    assert list(p)[1:] == ["scheme", "sk", "rnd", "m", "wire"] and p["wire"].default is False
    p = inspect.signature(Engine.public_keys_fixed).parameters
    assert list(p)[1:] == ["scheme", "sk", "wire"] and p["wire"].default is False
    for member in ("from_bytes", "to_bytes", "public_key", "public_key_double", "sign", "sign_double", "sign_batch", "sign_double_batch",
                   "with_variable_generator"):
        assert callable(getattr(SecretKey, member)), member
    assert "NOT constant time" in SecretKey.__doc__ and "NOT constant time" in Engine.sign_fixed.__doc__
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for needle in ("NOT constant time", "n_sk is n (a key per item) or 1", "any other value gives -1", "JJS_SCHEME_VARGEN and anything else give -1",
                   "A refused call writes nothing", "Rp_out and PKp_out must be NULL for the single"):
        assert needle in text, needle
    prof = open(os.path.join(ROOT, "include", "jjs_gpu_profiling.h")).read()
    assert "0x400000" in prof and "0x800000" in prof
    for name in ("sign_fixed.h", "sign_fixed_calls.h"):
        assert "NOT constant time" in open(os.path.join(ROOT, "jubjub_schnorr_amd", "csrc", name)).read(), name
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    for needle in ("class SecretKey {", "public_key_double", "sign_double_batch", "jjs_sign_fixed", "jjs_public_keys_fixed"):
        assert needle in hpp, needle

"""The extended-coordinate and host-buffer forms of the multisignature calls in the C ABI and its Python mirror: exported,
bound, -4 before jjs_init, and `fmt` accepted by the mirrors.  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
SYMBOLS = ("jjs_multisig_combine_ext_dev", "jjs_msig_group_create_ext", "jjs_msig_group_combine_ext_dev", "jjs_multisig_combine",
           "jjs_msig_group_combine")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_five_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    raw = ctypes.CDLL(LIB)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES and getattr(lib, name).argtypes == _ffi.SIGNATURES[name], name
    assert _ffi.SIGNATURES["jjs_multisig_combine_ext_dev"] == _ffi.SIGNATURES["jjs_multisig_combine_dev"]
    assert _ffi.SIGNATURES["jjs_msig_group_combine_ext_dev"] == _ffi.SIGNATURES["jjs_msig_group_combine_dev"]
    assert _ffi.SIGNATURES["jjs_msig_group_create_ext"] == _ffi.SIGNATURES["jjs_msig_group_create"]
    assert len(_ffi.SIGNATURES["jjs_multisig_combine"]) == 13 and len(_ffi.SIGNATURES["jjs_msig_group_combine"]) == 11
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    h = ctypes.c_uint64(0)
    assert lib.jjs_multisig_combine_ext_dev(*[None] * 6, 1, *[None] * 6) == -4
    assert lib.jjs_msig_group_create_ext(None, 1, ctypes.byref(h)) == -4
    assert lib.jjs_msig_group_combine_ext_dev(1, *[None] * 4, 1, *[None] * 5) == -4
    for fmt in (0, 1, 2):
        assert lib.jjs_multisig_combine(fmt, *[None] * 6, 1, *[None] * 5) == -4
        assert lib.jjs_msig_group_combine(1, fmt, *[None] * 4, 1, *[None] * 4) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_mirrors_take_fmt():
    from jubjub_schnorr_amd.api import Engine, SignerGroup
    for fn in (Engine.multisig_combine, Engine.multisig_group, SignerGroup.combine, SignerGroup.__init__):
        p = inspect.signature(fn).parameters
        assert "fmt" in p and p["fmt"].default == "affine", fn.__qualname__
    with pytest.raises(ValueError):
        Engine._msig_width("wire")
    assert Engine._msig_width("ext") == 96 and Engine._msig_width("affine") == 64


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(" in text, name
    assert "NOT InvalidPoint" in text, "the header says that Z = 0 is status 3 in the multisignature calls"

"""The wire forms of the multisignature calls in the C ABI and its Python mirror: the thirteen symbols exported, bound and
declared, -4 before jjs_init, the ABI version unchanged, the Python methods present, and `Engine._msig_width` still refusing
"wire" (the `format` argument of the existing calls keeps its meaning).  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
# name -> its affine twin, and what the twin's argument list loses (`format`) and merges (u, R -> sig_w) to give the wire form
TWINS = {
    "jjs_multisig_combine_wire_dev": ("jjs_multisig_combine_dev", 0, 0),
    "jjs_multisig_combine_wire": ("jjs_multisig_combine", 1, 0),
    "jjs_msig_group_create_wire": ("jjs_msig_group_create", 0, 0),
    "jjs_msig_group_combine_wire_dev": ("jjs_msig_group_combine_dev", 0, 0),
    "jjs_msig_group_combine_wire": ("jjs_msig_group_combine", 1, 0),
    "jjs_multisig_combine_keyset_wire_dev": ("jjs_multisig_combine_keyset_dev", 1, 0),
    "jjs_multisig_combine_keyset_wire": ("jjs_multisig_combine_keyset", 1, 0),
    "jjs_multisig_aggregate_pk_wire_dev": ("jjs_multisig_aggregate_pk_dev", 1, 0),
    "jjs_multisig_aggregate_pk_wire": ("jjs_multisig_aggregate_pk", 1, 0),
    "jjs_multisig_verify_wire_dev": ("jjs_multisig_verify_dev", 1, 1),
    "jjs_multisig_verify_wire": ("jjs_multisig_verify", 1, 1),
    "jjs_multisig_verify_keyset_wire_dev": ("jjs_multisig_verify_keyset_dev", 1, 1),
    "jjs_multisig_verify_keyset_wire": ("jjs_multisig_verify_keyset", 1, 1),
}
SYMBOLS = tuple(TWINS)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_thirteen_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    assert len(SYMBOLS) == 13
    raw = ctypes.CDLL(LIB)
    for name, (twin, formats, merged) in TWINS.items():
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES and getattr(lib, name).argtypes == _ffi.SIGNATURES[name], name
        want = list(_ffi.SIGNATURES[twin])
        if formats:
            want.remove(ctypes.c_int)
        if merged:
            want.remove(ctypes.c_void_p)
        assert _ffi.SIGNATURES[name] == want, (name, "the argument list of its affine twin")
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_minus_four_before_init(lib):
    from jubjub_schnorr_amd import _ffi
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    h = ctypes.c_uint64(0)
    for name in SYMBOLS:
        args = [1 if a in (ctypes.c_size_t, ctypes.c_uint64) else None for a in _ffi.SIGNATURES[name]]
        if name == "jjs_msig_group_create_wire":
            args[2] = ctypes.byref(h)
        assert getattr(lib, name)(*args) == -4, name
        assert b"jjs_init" in lib.jjs_last_error(), name
    for fmt in (0, 1, 2):                          # the calls that take a format answer -4 first, as before
        assert lib.jjs_multisig_combine(fmt, *[None] * 6, 1, *[None] * 5) == -4


def test_the_python_methods_exist():
    from jubjub_schnorr_amd.api import Engine, KeySet, SignerGroup
    for cls, names in ((Engine, ("multisig_combine_wire", "multisig_aggregate_pk_wire", "multisig_verify_wire", "multisig_group_wire")),
                       (SignerGroup, ("combine_wire",)), (KeySet, ("multisig_combine_wire", "multisig_verify_wire"))):
        for name in names:
            fn = getattr(cls, name)
            assert callable(fn) and "fmt" not in inspect.signature(fn).parameters, (cls.__name__, name)
    assert list(inspect.signature(Engine.multisig_verify_wire).parameters)[1:5] == ["PK_w", "offsets", "sig_w", "m"]
    with pytest.raises(ValueError):
        Engine._msig_width("wire")
    assert Engine._msig_width("ext") == 96 and Engine._msig_width("affine") == 64


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "jjs_gpu.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(" in text, name
    section = text.index("multisignature from wire encodings")
    assert text.index("multisignature from extended coordinates") < section < text.index("jjs_multisig_combine_wire_dev(")
    assert "64 bytes of 0xFF" in text[section:] and "JJS_FORMAT_WIRE with -1" in text[section:]
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    for name in ("jjs_multisig_combine_wire(", "jjs_multisig_aggregate_pk_wire(", "jjs_multisig_verify_wire(", "jjs_msig_group_create_wire(",
                 "jjs_msig_group_combine_wire("):
        assert name in hpp, name
    assert len(re.findall(r"_wire(_dev)?\(", text[section:text.index("multisignature for committees")])) >= 13

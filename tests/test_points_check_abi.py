"""jjs_keys_check(_dev) and jjs_signatures_check(_dev) in the C ABI and its mirrors: exported, bound with the signatures of
include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the Python mirror there.  No GPU: the library is loaded, never
initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
_P, _Z, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "jjs_keys_check_dev": [_I, _I, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_keys_check": [_I, _I, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_signatures_check_dev": [_I, _I, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_signatures_check": [_I, _I, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
}
DECLARATIONS = [
    "int jjs_keys_check_dev(int scheme, int format, const void* K0, const void* K1, size_t n, void* status, void* tally, void* A0_out, "
    "void* A1_out, void* stream);",
    "int jjs_keys_check(int scheme, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint8_t* status, uint64_t tally[4], "
    "uint8_t* A0_out, uint8_t* A1_out);",
    "int jjs_signatures_check_dev(int scheme, int format, const void* s0, const void* s1, const void* s2, size_t n, void* status, "
    "void* tally, void* u_out, void* R_out, void* Rp_out, void* stream);",
    "int jjs_signatures_check(int scheme, int format, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, size_t n, "
    "uint8_t* status, uint64_t tally[4], uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out);",
]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_four_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    raw = ctypes.CDLL(LIB)
    for name, sig in SYMBOLS.items():
        assert hasattr(raw, name), name
        assert _ffi.SIGNATURES.get(name) == sig and getattr(lib, name).argtypes == sig, name
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_the_header_declares_them():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "jjs_gpu.h")).read())
    for d in DECLARATIONS:
        assert d in text, d
    # no debug entry point was added for them (tests/test_abi.py pins the list)
    for h in ("jjs_gpu.h", "jjs_gpu_profiling.h"):
        assert not re.search(r"jjs_debug_\w*(check|valid)", open(os.path.join(ROOT, "include", h)).read())


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for scheme in (0, 1, 2, 7):
        for fmt in (0, 1, 2, 7):
            for n in (0, 1):
                assert lib.jjs_keys_check_dev(scheme, fmt, None, None, n, None, None, None, None, None) == -4
                assert lib.jjs_keys_check(scheme, fmt, None, None, n, None, None, None, None) == -4
                assert lib.jjs_signatures_check_dev(scheme, fmt, None, None, None, n, None, None, None, None, None, None) == -4
                assert lib.jjs_signatures_check(scheme, fmt, None, None, None, n, None, None, None, None, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_python_mirror():
    from jubjub_schnorr_amd import api
    for name in ("keys_check", "signatures_check"):
        p = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(p)[1:] == ["scheme", "cols", "fmt", "want_points"], name
        assert p["cols"].kind is inspect.Parameter.VAR_POSITIONAL and p["fmt"].default == "affine" and p["want_points"].default is False
    for cls in (api.PublicKey, api.PublicKeyDouble, api.PublicKeyVarGen, api.Signature, api.SignatureDouble, api.SignatureVarGen):
        assert callable(getattr(cls, "is_valid")), cls
        assert isinstance(inspect.getattr_static(cls, "is_valid_batch"), staticmethod), cls
        assert len(cls.is_valid_batch([])) == 0 and cls.is_valid_batch([]).dtype == bool


def test_the_cpp_mirror_declares_them():
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    assert "jjs_keys_check(" in hpp and "jjs_signatures_check(" in hpp
    for t in ("PublicKey", "PublicKeyDouble", "PublicKeyVarGen", "Signature", "SignatureDouble", "SignatureVarGen", "ExtendedPoint", "PointBytes"):
        assert re.search(r"is_valid_batch\(const std::vector<%s>&" % t, hpp), t
    assert hpp.count("bool is_valid() const;") == 6

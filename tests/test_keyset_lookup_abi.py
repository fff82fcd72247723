"""The by-key calls against a registered key set in the C ABI and its mirrors: exported, bound with the signatures of
include/jjs_gpu.h, -4 before jjs_init, JJS_STATUS_KEY_NOT_IN_SET = 6, the ABI version unchanged, the Python and C++ mirrors
there.  No GPU: the library is loaded, never initialised."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
_P, _Z, _I, _H = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
SYMBOLS = {
    "jjs_keyset_find_dev": [_H, _I, _P, _P, _Z, _P, _P],
    "jjs_keyset_find": [_H, _I, _P, _P, _Z, _P],
    "jjs_keyset_verify_keys_dev": [_H, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_keyset_verify_keys": [_H, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
}
DECLARATIONS = [
    "int jjs_keyset_find_dev(jjs_keyset ks, int format, const void* K0, const void* K1, size_t n, void* idx_out, void* stream);",
    "int jjs_keyset_find(jjs_keyset ks, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint32_t* idx_out);",
    "int jjs_keyset_verify_keys_dev(jjs_keyset ks, int format, const void* K0, const void* K1, const void* s0, const void* s1, "
    "const void* s2, const void* m, size_t n, void* status, void* tally, void* idx_out, void* stream);",
    "int jjs_keyset_verify_keys(jjs_keyset ks, int format, const uint8_t* K0, const uint8_t* K1, const uint8_t* s0, const uint8_t* s1, "
    "const uint8_t* s2, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4], uint32_t* idx_out);",
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
    # the by-index call's arguments with the key columns in place of key_idx, and the indices as a last output
    assert _ffi.SIGNATURES["jjs_keyset_verify_keys"][3:-1] == _ffi.SIGNATURES["jjs_keyset_verify"][2:]
    assert _ffi.SIGNATURES["jjs_keyset_verify_keys_dev"][3:-2] == _ffi.SIGNATURES["jjs_keyset_verify_dev"][2:-1]
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_the_header_declares_them_and_the_status():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "jjs_gpu.h")).read())
    for d in DECLARATIONS:
        assert d in text, d
    assert "#define JJS_STATUS_KEY_NOT_IN_SET 6" in text
    # the debug entry points are the ones that were there (tests/test_abi.py pins the list): none was added for the lookup
    for h in ("jjs_gpu.h", "jjs_gpu_profiling.h"):
        assert not re.search(r"jjs_debug_\w*(lookup|find|probe)", open(os.path.join(ROOT, "include", h)).read())


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for fmt in (0, 1, 2):
        for n in (0, 1):
            assert lib.jjs_keyset_find_dev(1, fmt, None, None, n, None, None) == -4
            assert lib.jjs_keyset_find(1, fmt, None, None, n, None) == -4
            assert lib.jjs_keyset_verify_keys_dev(1, fmt, *[None] * 6, n, None, None, None, None) == -4
            assert lib.jjs_keyset_verify_keys(1, fmt, *[None] * 6, n, None, None, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_python_mirror():
    from jubjub_schnorr_amd.api import KeySet
    p = inspect.signature(KeySet.find).parameters
    assert list(p)[1:] == ["keys", "fmt"] and p["keys"].kind is inspect.Parameter.VAR_POSITIONAL and p["fmt"].default == "affine"
    p = inspect.signature(KeySet.verify_keys).parameters
    assert list(p)[1:] == ["keys", "cols", "fmt", "want_status", "want_idx"] and p["fmt"].default == "affine"
    assert KeySet.NOT_IN_SET == 6 and KeySet.MISS == 0xFFFFFFFF


def test_the_cpp_mirror_compiles(tmp_path):
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    assert "jjs_keyset_find(" in hpp and "jjs_keyset_verify_keys(" in hpp
    src = tmp_path / "by_key.cpp"
    src.write_text('#include "jjs_schnorr.hpp"\n'
                   "std::vector<jjs::VerifyResult> by_key(const jjs::KeySet& ks, const std::vector<jjs::PublicKey::Item>& items, uint64_t* t) {\n"
                   "    return ks.verify(items, t);\n}\n"
                   "std::vector<uint32_t> where(const jjs::KeySet& ks, const std::vector<jjs::PublicKey>& keys) { return ks.find(keys); }\n"
                   "void raw(const jjs::KeySet& ks, const uint8_t* p, uint8_t* st, uint32_t* idx) {\n"
                   "    ks.find(JJS_FORMAT_WIRE, p, nullptr, 1, idx);\n"
                   "    ks.verify_keys(JJS_FORMAT_EXT, p, p, p, p, p, p, 1, st, nullptr, idx);\n}\n"
                   "static_assert(JJS_STATUS_KEY_NOT_IN_SET == 6, \"\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src)])

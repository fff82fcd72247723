"""jjs_keyset_add, jjs_keyset_reserve and jjs_keyset_growth in the C ABI and its mirrors: exported, bound with the signatures
of include/jjs_gpu.h, -4 before jjs_init, the mode and growth words of the header, the ABI version and JJS_KEYSET_INFO unchanged,
the Python and C++ mirrors there.  No GPU: the library is loaded, never initialised (the argument errors of an initialised
engine are tests/test_keyset_add_gpu.py's)."""
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
    "jjs_keyset_add": [_H, _I, _P, _P, _Z, _I, _P, _P, _P],
    "jjs_keyset_reserve": [_H, _Z],
    "jjs_keyset_growth": [_H, _P],
}
DECLARATIONS = [
    "int jjs_keyset_add(jjs_keyset ks, int format, const uint8_t* keys, const uint8_t* keys2, size_t n, int mode, uint8_t* key_status, "
    "uint32_t* idx_out, size_t* n_added);",
    "int jjs_keyset_reserve(jjs_keyset ks, size_t n_keys_total);",
    "int jjs_keyset_growth(jjs_keyset ks, uint64_t out[JJS_KEYSET_GROWTH]);",
]
DEFINES = {"JJS_KEYSET_ADD_APPEND": 0, "JJS_KEYSET_ADD_UNIQUE": 1, "JJS_KEYSET_CAPACITY": 0, "JJS_KEYSET_ADD_CALLS": 1, "JJS_KEYSET_RELOCATIONS": 2,
           "JJS_KEYSET_LOOKUP_REBUILDS": 3, "JJS_KEYSET_ADD_KNOWN": 4, "JJS_KEYSET_GROWTH": 5, "JJS_KEYSET_INFO": 7}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_three_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    raw = ctypes.CDLL(LIB)
    for name, sig in SYMBOLS.items():
        assert hasattr(raw, name), name
        assert _ffi.SIGNATURES.get(name) == sig and getattr(lib, name).argtypes == sig, name
    # the key columns and the status output of jjs_keyset_create, behind a handle instead of a scheme
    assert _ffi.SIGNATURES["jjs_keyset_add"][1:5] == _ffi.SIGNATURES["jjs_keyset_create"][1:5]
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_the_header_declares_them_and_their_words():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "jjs_gpu.h")).read())
    for d in DECLARATIONS:
        assert d in text, d
    for name, value in DEFINES.items():
        assert re.search(rf"#define {name} {value}\b", text), name
    for h in ("jjs_gpu.h", "jjs_gpu_profiling.h"):
        assert not re.search(r"jjs_debug_\w*(add|grow|reserve_keys)", open(os.path.join(ROOT, "include", h)).read())


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for mode in (0, 1, 2):
        for n in (0, 1):
            assert lib.jjs_keyset_add(1, 0, None, None, n, mode, None, None, None) == -4
    for total in (0, 1, 1 << 25):
        assert lib.jjs_keyset_reserve(1, total) == -4
    assert lib.jjs_keyset_growth(1, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_python_mirror():
    from jubjub_schnorr_amd.api import KeySet
    p = inspect.signature(KeySet.add).parameters
    assert list(p)[1:] == ["keys", "keys2", "fmt", "unique"] and p["keys2"].default is None and p["fmt"].default == "affine" and p["unique"].default is False
    assert list(inspect.signature(KeySet.reserve).parameters)[1:] == ["n"]
    assert KeySet.GROWTH_NAMES == ("capacity", "add_calls", "relocations", "lookup_rebuilds", "add_known")
    assert len(KeySet.INFO_NAMES) == 7


def test_the_cpp_mirror_compiles(tmp_path):
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    assert "jjs_keyset_add(" in hpp and "jjs_keyset_reserve(" in hpp and "jjs_keyset_growth(" in hpp
    src = tmp_path / "grow.cpp"
    src.write_text('#include "jjs_schnorr.hpp"\n'
                   "jjs::KeySet::Added more(jjs::KeySet& ks, const std::vector<jjs::PublicKey>& keys) { return ks.add(keys, true); }\n"
                   "void raw(jjs::KeySet& ks, const uint8_t* p) {\n"
                   "    ks.reserve(100);\n"
                   "    jjs::KeySet::Added a = ks.add(JJS_FORMAT_WIRE, p, nullptr, 1);\n"
                   "    (void)a.n_added; (void)ks.growth()[JJS_KEYSET_RELOCATIONS];\n}\n"
                   "static_assert(JJS_KEYSET_GROWTH == 5 && JJS_KEYSET_INFO == 7 && JJS_KEYSET_ADD_UNIQUE == 1, \"\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src)])

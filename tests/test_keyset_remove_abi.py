"""jjs_keyset_remove, jjs_keyset_compact and jjs_keyset_removal in the C ABI and its mirrors: exported, bound with the signatures
of include/jjs_gpu.h, -4 before jjs_init, the result and removal words of the header, the ABI version, JJS_KEYSET_INFO and
JJS_KEYSET_GROWTH unchanged, the Python and C++ mirrors there.  No GPU: the library is loaded, never initialised (the argument
errors of an initialised engine are tests/test_keyset_remove_gpu.py's)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
_P, _Z, _H = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
SYMBOLS = {
    "jjs_keyset_remove": [_H, _P, _Z, _P, _P],
    "jjs_keyset_compact": [_H, _P, _Z, _P],
    "jjs_keyset_removal": [_H, _P],
}
DECLARATIONS = [
    "int jjs_keyset_remove(jjs_keyset ks, const uint32_t* idx, size_t n, uint8_t* result, size_t* n_removed);",
    "int jjs_keyset_compact(jjs_keyset ks, uint32_t* map_out, size_t map_len, size_t* n_keys_out);",
    "int jjs_keyset_removal(jjs_keyset ks, uint64_t out[JJS_KEYSET_REMOVAL]);",
]
DEFINES = {"JJS_KEY_WAS_REMOVED": "8", "JJS_KEY_NOT_IN_RANGE": "0xFF", "JJS_KEYSET_REMOVED_KEYS": "0", "JJS_KEYSET_LIVE_KEYS": "1",
           "JJS_KEYSET_REMOVE_CALLS": "2", "JJS_KEYSET_COMPACT_CALLS": "3", "JJS_KEYSET_REMOVAL": "4", "JJS_KEYSET_INFO": "7",
           "JJS_KEYSET_GROWTH": "5"}


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
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_the_header_declares_them_and_their_words():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "jjs_gpu.h")).read())
    for d in DECLARATIONS:
        assert d in text, d
    for name, value in DEFINES.items():
        assert re.search(rf"#define {name} {value}\b", text), name
    for h in ("jjs_gpu.h", "jjs_gpu_profiling.h"):
        assert not re.search(r"jjs_debug_\w*(remove|compact)", open(os.path.join(ROOT, "include", h)).read())


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    idx = (ctypes.c_uint32 * 2)(0, 1)
    for n in (0, 2):
        assert lib.jjs_keyset_remove(1, idx, n, None, None) == -4
        assert lib.jjs_keyset_remove(1, None, n, None, None) == -4
    for map_len in (0, 2):
        assert lib.jjs_keyset_compact(1, None, map_len, None) == -4
        assert lib.jjs_keyset_compact(1, idx, map_len, None) == -4
    assert lib.jjs_keyset_removal(1, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_python_mirror():
    from jubjub_schnorr_amd.api import KeySet
    assert list(inspect.signature(KeySet.remove).parameters)[1:] == ["idx"]
    assert list(inspect.signature(KeySet.compact).parameters)[1:] == []
    assert KeySet.REMOVAL_NAMES == ("removed_keys", "live_keys", "remove_calls", "compact_calls")
    assert (KeySet.WAS_REMOVED, KeySet.NOT_IN_RANGE) == (8, 0xFF) and isinstance(KeySet.removed, property)
    assert len(KeySet.INFO_NAMES) == 7 and len(KeySet.GROWTH_NAMES) == 5


def test_the_cpp_mirror_compiles(tmp_path):
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    assert "jjs_keyset_remove(" in hpp and "jjs_keyset_compact(" in hpp and "jjs_keyset_removal(" in hpp
    src = tmp_path / "shrink.cpp"
    src.write_text('#include "jjs_schnorr.hpp"\n'
                   "std::vector<uint32_t> drop(jjs::KeySet& ks, const std::vector<uint32_t>& idx) {\n"
                   "    jjs::KeySet::Removed r = ks.remove(idx);\n"
                   "    (void)r.n_removed; (void)r.result.size(); (void)ks.removal()[JJS_KEYSET_LIVE_KEYS];\n"
                   "    return ks.compact();\n}\n"
                   "static_assert(JJS_KEYSET_REMOVAL == 4 && JJS_KEYSET_GROWTH == 5 && JJS_KEYSET_INFO == 7 && JJS_KEY_WAS_REMOVED == 8, \"\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src)])

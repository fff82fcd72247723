"""jjs_digest(_dev) and jjs_debug_digest_limits in the C ABI and its mirrors: exported, bound with the signatures of
include/jjs_gpu.h, -4 before jjs_init, the ABI version unchanged, the Python and C++ mirrors there.  No GPU: the library is loaded,
never initialised."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jubjub_schnorr_amd", "libjjs_gpu.so")
_P, _Z, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "jjs_digest_dev": [_I, _I, _P, _P, _Z, _Z, _P, _P, _P],
    "jjs_digest": [_I, _I, _P, _P, _Z, _Z, _P, _P],
    "jjs_debug_digest_limits": [_P],
}
DECLARATIONS = [
    "int jjs_digest_dev(int format, int flags, const void* in, const uint32_t* offsets_host, size_t k, size_t n, void* out, void* status, "
    "void* stream);",
    "int jjs_digest(int format, int flags, const uint8_t* in, const uint32_t* offsets, size_t k, size_t n, uint8_t* out, uint8_t* status);",
    "int jjs_debug_digest_limits(uint64_t out[2]);",
    "#define JJS_DIGEST_CANONICAL 0", "#define JJS_DIGEST_WIDE 1", "#define JJS_DIGEST_TRUNCATED 1",
]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def test_the_symbols_are_exported_and_bound(lib):
    from jubjub_schnorr_amd import _ffi
    raw = ctypes.CDLL(LIB)
    for name, sig in SYMBOLS.items():
        assert hasattr(raw, name), name
        assert _ffi.SIGNATURES.get(name) == sig and getattr(lib, name).argtypes == sig, name
    assert lib.jjs_abi_version() == 5, "the additions are additive"


def test_the_header_declares_them():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "jjs_gpu.h")).read())
    text = re.sub(r"/\*.*?\*/", "", text)
    text = re.sub(r"\s+", " ", text)
    for d in DECLARATIONS:
        assert d in text, d
    # the switches that choose a route live in the profiling build alone, behind the entry point that is there already
    prof = open(os.path.join(ROOT, "include", "jjs_gpu_profiling.h")).read()
    assert "jjs_digest" in prof and not re.search(r"jjs_debug_\w*digest", prof)


def test_minus_four_before_init(lib):
    assert lib.jjs_device_count() == 0, "this process must not have initialised the engine"
    for fmt in (0, 1, 7):
        for flags in (0, 1, 2):
            for n in (0, 1):
                assert lib.jjs_digest_dev(fmt, flags, None, None, 1, n, None, None, None) == -4
                assert lib.jjs_digest(fmt, flags, None, None, 1, n, None, None) == -4
    assert lib.jjs_debug_digest_limits(None) == -4
    assert b"jjs_init" in lib.jjs_last_error()


def test_the_python_mirror():
    from jubjub_schnorr_amd import api
    p = inspect.signature(api.Engine.digest).parameters
    assert list(p)[1:] == ["inputs", "lengths", "truncated", "fmt"]
    assert p["lengths"].default is None and p["truncated"].default is False and p["fmt"].default == "canonical"
    assert p["truncated"].kind is inspect.Parameter.KEYWORD_ONLY and p["fmt"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(api.Engine.digest_limits)


def test_the_cpp_mirror_declares_them():
    hpp = open(os.path.join(ROOT, "include", "jjs_schnorr.hpp")).read()
    assert "namespace poseidon {" in hpp and "jjs_digest(" in hpp
    for f in ("digest(const std::vector<BlsScalar>&", "digest_truncated(const std::vector<BlsScalar>&",
              "digest_batch(const std::vector<std::vector<BlsScalar>>&"):
        assert f in hpp, f


def test_the_generated_constant_of_the_wide_format():
    """JJS_TWO256 is what tools/gen_constants.py emits: 2^256 in Montgomery form, nine 29-bit limbs"""
    import jjs_oracle as o
    inc = open(os.path.join(ROOT, "jubjub_schnorr_amd", "csrc", "jjs_constants.inc")).read()
    m = re.search(r"JJS_TWO256\[9\] = \{([^}]*)\}", inc)
    limbs = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    assert len(limbs) == 9 and all(v < 1 << 29 for v in limbs)
    assert sum(v << (29 * i) for i, v in enumerate(limbs)) == (1 << 256) * (1 << 261) % o.Q

"""Registered key sets (include/jjs_gpu.h jjs_keyset_*) without a GPU: the declared surface, the binding, the exports and the
not-initialised contract; the CPU build of csrc/keyset.h against the oracle is tests/test_keyset_host.py."""
import ctypes
import os

import pytest

from test_abi import exported, header_symbols

KEYSET_FUNCS = ["jjs_keyset_create", "jjs_keyset_destroy", "jjs_keyset_info", "jjs_keyset_verify", "jjs_keyset_verify_dev"]


def test_header_declares_the_keyset_functions_and_the_binding_mirrors_them():
    from jubjub_schnorr_amd import _ffi
    syms = header_symbols()
    for s in KEYSET_FUNCS:
        assert s in syms
        assert s in _ffi.SIGNATURES
    assert not any(w in s for s in KEYSET_FUNCS for w in ("skip", "virtual", "force", "fail", "pin_"))


def test_library_exports_the_keyset_functions():
    from jubjub_schnorr_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run __graft_entry__.build()")
    assert set(KEYSET_FUNCS) <= exported(_ffi.LIB_PATH)


def test_keyset_calls_before_init_report_not_initialised():
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    lib.jjs_shutdown()
    h = ctypes.c_uint64(0)
    keys = (ctypes.c_uint8 * 64)()
    out = (ctypes.c_uint64 * 7)()
    assert lib.jjs_keyset_create(0, 0, keys, None, 1, None, ctypes.byref(h)) == -4
    assert h.value == 0
    assert lib.jjs_keyset_destroy(1 << 32 | 1) == -4
    assert lib.jjs_keyset_info(1 << 32 | 1, out) == -4
    assert lib.jjs_keyset_verify(1 << 32 | 1, 0, None, None, None, None, None, 0, None, None) == -4
    assert lib.jjs_keyset_verify_dev(1 << 32 | 1, 0, None, None, None, None, None, 0, None, None, None) == -4
    assert b"jjs_init" in lib.jjs_last_error()

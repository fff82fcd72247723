"""ctypes binding of libjjs_gpu.so (the C ABI declared in include/jjs_gpu.h).

There is no fallback: if the HIP library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# The product library.  No environment variable can redirect the loader; tools that need another in-tree build
# of the same sources (the -DJJS_PROFILING build, A/B variants of a kernel) call select_library() explicitly
# before the first use.
LIB_PATH = os.path.join(HERE, "libjjs_gpu.so")
PROFILING_LIB_PATH = os.path.join(HERE, "libjjs_gpu_prof.so")

_P, _Z, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int

# name -> argtypes (restype is int unless listed in _RESTYPES); mirrors include/jjs_gpu.h
SIGNATURES = {
    "jjs_init": [_I],
    "jjs_shutdown": [],
    "jjs_last_error": [],
    "jjs_abi_version": [],
    "jjs_device_count": [],
    "jjs_collective_ranks": [],
    "jjs_verify_single": [_P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_double": [_P, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_vargen": [_P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_single_dev": [_P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_double_dev": [_P, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_vargen_dev": [_P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_stream_sync": [_P],
    "jjs_path_stats": [_P],
    "jjs_reserve": [_I, _I, _Z, _I],
    "jjs_trim": [],
    "jjs_memory_stats": [_P],
    "jjs_verify_single_wire_dev": [_P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_double_wire_dev": [_P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_vargen_wire_dev": [_P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_single_wire": [_P, _P, _P, _Z, _P, _P],
    "jjs_verify_double_wire": [_P, _P, _P, _Z, _P, _P],
    "jjs_verify_vargen_wire": [_P, _P, _P, _Z, _P, _P],
    "jjs_verify_single_ext_dev": [_P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_double_ext_dev": [_P, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_vargen_ext_dev": [_P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_verify_single_ext": [_P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_double_ext": [_P, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_vargen_ext": [_P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_multisig_combine_dev": [_P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_decompress_dev": [_P, _Z, _P, _P, _P],
    "jjs_compress_dev": [_P, _Z, _P, _P],
    "jjs_challenge_single_dev": [_P, _P, _P, _Z, _P, _P],
    "jjs_challenge_double_dev": [_P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_challenge_vargen_dev": [_P, _P, _P, _P, _Z, _P, _P],
    "jjs_sign_single_dev": [_P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_sign_double_dev": [_P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_sign_vargen_dev": [_P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_debug_fq_mul_dev": [_P, _P, _Z, _P, _P],
    "jjs_debug_poseidon_dev": [_P, _Z, _Z, _P, _P],
    "jjs_debug_point_flags_dev": [_P, _Z, _P, _P],
    "jjs_debug_half_scalars_dev": [_P, _Z, _P, _P, _P, _P],
    "jjs_debug_comb_table_bytes": [],
    "jjs_debug_comb_table": [_I, _P],
    "jjs_debug_dlog_tables": [_P, _P],
    "jjs_debug_rccl_selftest": [],
    "jjs_debug_msig_resident_lanes": [],
    "jjs_public_keys_dev": [_P, _Z, _P, _P, _P, _P],
    "jjs_keyset_create": [_I, _I, _P, _P, _Z, _P, _P],
    "jjs_keyset_destroy": [ctypes.c_uint64],
    "jjs_keyset_info": [ctypes.c_uint64, _P],
    "jjs_keyset_verify": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_keyset_verify_dev": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_keyset_find_dev": [ctypes.c_uint64, _I, _P, _P, _Z, _P, _P],
    "jjs_keyset_find": [ctypes.c_uint64, _I, _P, _P, _Z, _P],
    "jjs_keyset_verify_keys_dev": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_keyset_verify_keys": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_keyset_add": [ctypes.c_uint64, _I, _P, _P, _Z, _I, _P, _P, _P],
    "jjs_keyset_reserve": [ctypes.c_uint64, _Z],
    "jjs_keyset_growth": [ctypes.c_uint64, _P],
    "jjs_keyset_remove": [ctypes.c_uint64, _P, _Z, _P, _P],
    "jjs_keyset_compact": [ctypes.c_uint64, _P, _Z, _P],
    "jjs_keyset_removal": [ctypes.c_uint64, _P],
    "jjs_keys_check_dev": [_I, _I, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_keys_check": [_I, _I, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_signatures_check_dev": [_I, _I, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_signatures_check": [_I, _I, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_keyset_verify_all": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_keyset_verify_all_dev": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_msig_group_create": [_P, _Z, _P],
    "jjs_msig_group_destroy": [ctypes.c_uint64],
    "jjs_msig_group_info": [ctypes.c_uint64, _P],
    "jjs_msig_group_aggregate_pk": [ctypes.c_uint64, _P],
    "jjs_msig_group_combine_dev": [ctypes.c_uint64, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_multisig_combine_ext_dev": [_P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_msig_group_create_ext": [_P, _Z, _P],
    "jjs_msig_group_combine_ext_dev": [ctypes.c_uint64, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_multisig_combine": [_I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_msig_group_combine": [ctypes.c_uint64, _I, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_combine_keyset_dev": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_multisig_combine_keyset": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_multisig_aggregate_pk_dev": [_I, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_aggregate_pk": [_I, _P, _P, _Z, _P, _P],
    "jjs_multisig_aggregate_pk_keyset_dev": [ctypes.c_uint64, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_aggregate_pk_keyset": [ctypes.c_uint64, _P, _P, _Z, _P, _P],
    "jjs_multisig_verify_dev": [_I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_verify": [_I, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_verify_keyset_dev": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_verify_keyset": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P, _P],
    # the wire forms: the argument list of the affine twin, without `format`, with the one sig_w column where the twin has u, R
    "jjs_multisig_combine_wire_dev": [_P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_multisig_combine_wire": [_P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_msig_group_create_wire": [_P, _Z, _P],
    "jjs_msig_group_combine_wire_dev": [ctypes.c_uint64, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_msig_group_combine_wire": [ctypes.c_uint64, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_combine_keyset_wire_dev": [ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_multisig_combine_keyset_wire": [ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_multisig_aggregate_pk_wire_dev": [_P, _P, _Z, _P, _P, _P],
    "jjs_multisig_aggregate_pk_wire": [_P, _P, _Z, _P, _P],
    "jjs_multisig_verify_wire_dev": [_P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_verify_wire": [_P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_verify_keyset_wire_dev": [ctypes.c_uint64, _P, _P, _P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_verify_keyset_wire": [ctypes.c_uint64, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_round1_dev": [_P, _P, _Z, _P, _P, _P, _P],
    "jjs_multisig_sign_dev": [_I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_sign": [_I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _Z, _P, _P],
    # verify_share on its own: the transcripts of the route's combine call, then share_transcript, share_slot, z, n_shares, the outputs
    "jjs_multisig_verify_share_dev": [_I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_verify_share": [_I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P],
    "jjs_msig_group_verify_share_dev": [ctypes.c_uint64, _I, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_msig_group_verify_share": [ctypes.c_uint64, _I, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P],
    "jjs_multisig_verify_share_keyset_dev": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_multisig_verify_share_keyset": [ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P],
    "jjs_public_keys_vargen_dev": [_I, _P, _P, _Z, _Z, _P, _P, _P, _P],
    "jjs_sign_vargen_pt_dev": [_I, _P, _P, _Z, _P, _P, _Z, _P, _P, _P, _P, _P, _P],
    "jjs_public_keys_vargen": [_I, _P, _P, _Z, _Z, _P, _P, _P],
    "jjs_sign_vargen_pt": [_I, _P, _P, _Z, _P, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_debug_sign_limits": [_P],
    "jjs_sign_fixed_dev": [_I, _P, _Z, _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "jjs_sign_fixed": [_I, _P, _Z, _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P, _P],
    "jjs_public_keys_fixed_dev": [_I, _P, _Z, _P, _P, _P, _P, _P],
    "jjs_public_keys_fixed": [_I, _P, _Z, _P, _P, _P, _P],
    "jjs_debug_sign_fixed_limits": [_P],
    "jjs_digest_dev": [_I, _I, _P, _P, _Z, _Z, _P, _P, _P],
    "jjs_digest": [_I, _I, _P, _P, _Z, _Z, _P, _P],
    "jjs_debug_digest_limits": [_P],
    "jjs_verify_all_single": [_P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_all_double": [_P, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_all_vargen": [_P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_all_single_dev": [_P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_all_double_dev": [_P, _P, _P, _P, _P, _P, _Z, _P, _P],
    "jjs_verify_all_vargen_dev": [_P, _P, _P, _P, _P, _Z, _P, _P],
}
# include/jjs_gpu_profiling.h: present in libjjs_gpu_prof.so only
PROFILING_SIGNATURES = {
    "jjs_debug_skip_phases": [ctypes.c_uint],
    "jjs_debug_allow_virtual_devices": [_I],
    "jjs_debug_force_path": [_I],
    "jjs_debug_host_timing": [_P],
    "jjs_debug_fail_key_arena": [_I],
    "jjs_debug_pin_hash_seed": [_I],
    "jjs_debug_msm_dev": [_P, _P, _Z, ctypes.c_uint, ctypes.c_uint, _I, _I, _P, _P, _P, _P, _P],
    "jjs_debug_keyset_sums_dev": [ctypes.c_uint64, _P, _P, _P, _Z, _P, _P, _P],
    "jjs_debug_verdict_items_dev": [_I, _P, _P, _P, _P, _P, _P, _Z, _I, ctypes.c_uint, _P, _P, _P, _P, _P, _P],
    "jjs_debug_keyset_items_dev": [ctypes.c_uint64, _P, _P, _P, _P, _P, _Z, _I, ctypes.c_uint, _P, _P, _P, _P, _P, _P, _P, _P],
}
_RESTYPES = {"jjs_shutdown": None, "jjs_last_error": ctypes.c_char_p, "jjs_debug_comb_table_bytes": _Z}


class JjsError(RuntimeError):
    pass


_lib = None


def select_library(path: str) -> None:
    """Load another in-tree build of the engine instead of libjjs_gpu.so (profiling build, A/B kernel variants).
    Only before the first use, and only a libjjs_gpu*.so inside this package directory."""
    global LIB_PATH
    path = os.path.abspath(path)
    if _lib is not None:
        raise JjsError("select_library() must be called before the library is first used")
    if os.path.dirname(path) != HERE or not os.path.basename(path).startswith("libjjs_gpu"):
        raise JjsError(f"{path}: not an in-tree build of the engine")
    LIB_PATH = path


def lib():
    """The loaded library with typed entry points.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JjsError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # If PyTorch is going to share the process it must be loaded first: it ships its own libamdhip64
        # (same SONAME), and the dynamic loader then binds this library to that copy, so that both see
        # one HIP runtime (one current device, shared device pointers and streams).  Loaded the other
        # way round torch finds no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the ABI and the header diverge
            fn.argtypes = args
            fn.restype = _RESTYPES.get(name, _I)
        for name, args in PROFILING_SIGNATURES.items():
            if hasattr(l, name):   # the profiling build only
                getattr(l, name).argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().jjs_last_error()
        raise JjsError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")

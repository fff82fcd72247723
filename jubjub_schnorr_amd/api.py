"""Host-side interface over libjjs_gpu.so.

Two levels:

* `Engine`: batch calls on torch CUDA tensors (resident data; asynchronous on torch's current
  stream) or numpy arrays (host buffers; blocking).  Arrays are uint8, SoA: scalars / field
  elements (n, 32) little-endian canonical; points (n, 64) = affine u || v.
* `PublicKey` / `Signature` & co.: the reference crate's types and method names
  (`PublicKey::verify(&self, &Signature, BlsScalar) -> Result<(), Error>`, reference
  src/keys/public.rs:114; `PublicKeyDouble::verify` src/keys/public/double.rs:86;
  `PublicKeyVarGen::verify` src/keys/public/var_gen.rs:107) plus the batch entry point a shim would
  add (`verify_batch`).  Errors mirror reference src/error.rs:13-19.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import _ffi

STATUS_NAMES = ("Ok", "InvalidPoint", "InvalidSignature", "Malformed")


class Error(Exception):
    """Base of the reference's `Error` enum variants reachable from verify."""


class InvalidPoint(Error):
    def __str__(self):
        return "Invalid Point"


class InvalidSignature(Error):
    def __str__(self):
        return "Invalid Signature"


class Malformed(Error):
    """Non-canonical encoding; unreachable through the Rust types (their from_bytes rejects it)."""

    def __str__(self):
        return "Malformed encoding"


_ERRORS = {1: InvalidPoint, 2: InvalidSignature, 3: Malformed}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class Engine:
    """One engine per process.  `device_count=1` (default) binds it to the current HIP device -- one process
    per GPU, what a torch.distributed rank uses; `device_count=k` drives devices 0..k-1 and 0 every visible
    device from this one process: the numpy (host-buffer) calls are then sharded across them by the library."""

    def __init__(self, device_count: int = 1):
        # When PyTorch shares the process, let it bring up the HIP runtime first: torch ships its own
        # libamdhip64 and fails with "No HIP GPUs are available" if another copy initialised the device
        # before it (observed on ROCm 7.2 / torch 2.10).
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        self._lib = _ffi.lib()
        _ffi.check(self._lib.jjs_init(int(device_count)), "jjs_init")
        self.device_count = self._lib.jjs_device_count()

    # ---- helpers ------------------------------------------------------------------------------
    @staticmethod
    def _dev_ptr(t, width, n=None):
        import torch
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise ValueError("expected a contiguous uint8 CUDA tensor")
        if t.dim() != 2 or t.shape[1] != width or (n is not None and t.shape[0] != n):
            raise ValueError(f"expected shape (n, {width}), got {tuple(t.shape)}")
        return ctypes.c_void_p(t.data_ptr())

    @staticmethod
    def _stream():
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _host(a, width):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(f"expected shape (n, {width}), got {a.shape}")
        return a

    _WIDTHS = {"single": (32, 64, 64, 32), "double": (32, 64, 64, 64, 64, 32), "vargen": (32, 64, 64, 64, 32)}

    def verify_ext(self, scheme: str, *arrays, want_status: bool = True):
        """Batch verify with every point in extended coordinates, (n, 96) = U || V || Z canonical (what the Rust
        `JubJubExtended` holds; normalised on the device).  Same argument order and results as `verify`."""
        return self.verify(scheme, *arrays, want_status=want_status, _ext=True)

    def verify(self, scheme: str, *arrays, want_status: bool = True, _ext: bool = False):
        """Batch verify.  Argument order per scheme: single (u, R, PK, m); double (u, R, R', PK, PK', m);
        vargen (u, R, PK, Gen, m).  Returns (status, tally): same kind as the inputs (torch CUDA
        tensors, asynchronous on the current stream, or numpy arrays, blocking)."""
        widths = self._WIDTHS[scheme]
        suffix = ""
        if _ext:
            widths = tuple(96 if w == 64 else w for w in widths)
            suffix = "_ext"
        if len(arrays) != len(widths):
            raise ValueError(f"{scheme} verify takes {len(widths)} arrays")
        if _is_torch(arrays[0]):
            import torch
            n = arrays[0].shape[0]
            ptrs = [self._dev_ptr(a, w, n) for a, w in zip(arrays, widths)]
            dev = arrays[0].device
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n] if want_status else None
            tally = torch.empty(4, dtype=torch.int64, device=dev)          # the call clears it (one launch fewer than torch.zeros)
            fn = getattr(self._lib, f"jjs_verify_{scheme}{suffix}_dev")
            _ffi.check(fn(*ptrs, n, ctypes.c_void_p(status.data_ptr()) if want_status and n else None,
                          ctypes.c_void_p(tally.data_ptr()), self._stream()), f"jjs_verify_{scheme}{suffix}_dev")
            return status, tally
        host = [self._host(a, w) for a, w in zip(arrays, widths)]
        n = host[0].shape[0]
        if any(h.shape[0] != n for h in host):
            raise ValueError("all arrays must have the same number of items")
        status = np.empty(n, np.uint8)
        tally = np.zeros(4, np.uint64)
        fn = getattr(self._lib, f"jjs_verify_{scheme}{suffix}")
        _ffi.check(fn(*[h.ctypes.data_as(ctypes.c_void_p) for h in host], n, status.ctypes.data_as(ctypes.c_void_p),
                      tally.ctypes.data_as(ctypes.c_void_p)), f"jjs_verify_{scheme}{suffix}")
        return status, tally

    def verify_all(self, scheme: str, *arrays, statuses_on_failure: bool = True):
        """One verdict for the whole batch (jjs_verify_all_*): True when every item would get status 0 from `verify`.
        Same arguments as `verify` (affine columns).  numpy inputs: blocking, returns (bool, status or None) -- the
        statuses of `verify`, byte for byte, when the verdict is False and `statuses_on_failure` is set.  torch CUDA
        tensors: asynchronous on the current stream, returns a device uint32 tensor of one element (1 accepted, 0 not);
        run `verify` for the statuses."""
        widths = self._WIDTHS[scheme]
        if len(arrays) != len(widths):
            raise ValueError(f"{scheme} verify_all takes {len(widths)} arrays")
        if _is_torch(arrays[0]):
            import torch
            n = arrays[0].shape[0]
            ptrs = [self._dev_ptr(a, w, n) for a, w in zip(arrays, widths)]
            verdict = torch.empty(1, dtype=torch.int32, device=arrays[0].device)
            fn = getattr(self._lib, f"jjs_verify_all_{scheme}_dev")
            _ffi.check(fn(*ptrs, n, ctypes.c_void_p(verdict.data_ptr()), self._stream()), f"jjs_verify_all_{scheme}_dev")
            return verdict.view(torch.uint32) if hasattr(torch, "uint32") else verdict
        host = [self._host(a, w) for a, w in zip(arrays, widths)]
        n = host[0].shape[0]
        if any(h.shape[0] != n for h in host):
            raise ValueError("all arrays must have the same number of items")
        status = np.empty(n, np.uint8) if statuses_on_failure else None
        verdict = ctypes.c_int(-1)
        fn = getattr(self._lib, f"jjs_verify_all_{scheme}")
        _ffi.check(fn(*[h.ctypes.data_as(ctypes.c_void_p) for h in host], n,
                      status.ctypes.data_as(ctypes.c_void_p) if status is not None else None, ctypes.byref(verdict)),
                   f"jjs_verify_all_{scheme}")
        ok = verdict.value == 1
        return ok, (None if ok or status is None else status)

    PATH_STAT_NAMES = ("latency", "throughput", "key_tables_wide", "key_tables_narrow", "keys_do_not_repeat",
                       "keys_probe_limit", "keys_pool_too_small", "keys_no_memory", "key_pool_bytes", "lane_launches", "lane_calls")

    def path_stats(self) -> dict:
        """Which method the calls on the current device took so far (jjs_path_stats): calls per path, and the bytes the
        per-key tables hold.  Calls still running are not in yet."""
        out = (ctypes.c_uint64 * len(self.PATH_STAT_NAMES))()
        _ffi.check(self._lib.jjs_path_stats(out), "jjs_path_stats")
        return dict(zip(self.PATH_STAT_NAMES, (int(v) for v in out)))

    _SCHEME_IDS = {"single": 0, "double": 1, "vargen": 2}
    _FORMAT_IDS = {"affine": 0, "ext": 1, "wire": 2}
    MEMORY_STAT_NAMES = ("key_pools", "slot_buffers", "host_staging", "retired")

    def reserve(self, scheme: str, n_items: int, fmt: str = "affine", host_buffers: bool = False) -> None:
        """Pre-size the engine for calls of this scheme, input format ("affine", "ext", "wire") and at most `n_items` items
        (jjs_reserve): no later call of that shape allocates.  `host_buffers`: also the staging of the numpy (blocking) calls."""
        _ffi.check(self._lib.jjs_reserve(self._SCHEME_IDS[scheme], self._FORMAT_IDS[fmt], int(n_items), int(bool(host_buffers))),
                   "jjs_reserve")

    def trim(self) -> None:
        """Wait for the device, free retired buffers and the key-table pools (jjs_trim)."""
        _ffi.check(self._lib.jjs_trim(), "jjs_trim")

    def memory_stats(self) -> dict:
        out = (ctypes.c_uint64 * len(self.MEMORY_STAT_NAMES))()
        _ffi.check(self._lib.jjs_memory_stats(out), "jjs_memory_stats")
        return dict(zip(self.MEMORY_STAT_NAMES, (int(v) for v in out)))

    _WIRE_WIDTHS = {"single": (64, 32, 32), "double": (96, 64, 32), "vargen": (64, 64, 32)}

    def keyset(self, scheme: str, keys, keys2=None, fmt: str = "affine") -> "KeySet":
        """Register keys once (jjs_keyset_create): validity and window tables are built on every driven device and kept
        until the set is closed.  affine / ext: `keys` (n, 64 | 96) is the first point column, `keys2` the second (PK' for
        double, the generator for vargen); wire: `keys` in the layout of `verify_wire`'s pk, `keys2` None."""
        return KeySet(self, scheme, keys, keys2, fmt)

    # ---- `is_valid` alone (include/jjs_gpu.h jjs_keys_check / jjs_signatures_check) ----------------------------------
    def _points_check(self, kind: str, scheme: str, cols, fmt: str, want_points: bool):
        two = (scheme != "single") if kind == "keys" else (scheme == "double")
        if kind == "keys":
            widths = [64 if two else 32] if fmt == "wire" else [96 if fmt == "ext" else 64] * (2 if two else 1)
            slots, out_widths = 2, [64] + ([64] if two else [])
        else:
            widths = [96 if two else 64] if fmt == "wire" else [32] + [96 if fmt == "ext" else 64] * (2 if two else 1)
            slots, out_widths = 3, [32, 64] + ([64] if two else [])
        if len(cols) != len(widths):
            raise ValueError(f"{scheme} {fmt} {kind} come in {len(widths)} column(s)")
        n_outs = slots                         # keys: A0, A1; signatures: u, R, R'
        ids = (self._SCHEME_IDS[scheme], self._FORMAT_IDS[fmt])
        n = cols[0].shape[0]
        if _is_torch(cols[0]):
            import torch
            dev = cols[0].device
            ptrs = [self._dev_ptr(c, w, n) for c, w in zip(cols, widths)] + [None] * (slots - len(cols))
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
            tally = torch.empty(4, dtype=torch.int64, device=dev)
            outs = [torch.empty((max(n, 1), w), dtype=torch.uint8, device=dev)[:n] for w in out_widths] if want_points else []
            optrs = [ctypes.c_void_p(a.data_ptr()) if n else None for a in outs] + [None] * (n_outs - len(outs))
            name = f"jjs_{kind}_check_dev"
            _ffi.check(getattr(self._lib, name)(*ids, *ptrs, n, ctypes.c_void_p(status.data_ptr()) if n else None,
                                                ctypes.c_void_p(tally.data_ptr()), *optrs, self._stream()), name)
        else:
            host = [self._host(c, w) for c, w in zip(cols, widths)]
            if any(h.shape[0] != n for h in host):
                raise ValueError("all columns must have the same number of items")
            ptrs = [h.ctypes.data_as(ctypes.c_void_p) for h in host] + [None] * (slots - len(cols))
            status, tally = np.empty(n, np.uint8), np.zeros(4, np.uint64)
            outs = [np.empty((n, w), np.uint8) for w in out_widths] if want_points else []
            optrs = [a.ctypes.data_as(ctypes.c_void_p) for a in outs] + [None] * (n_outs - len(outs))
            name = f"jjs_{kind}_check"
            _ffi.check(getattr(self._lib, name)(*ids, *ptrs, n, status.ctypes.data_as(ctypes.c_void_p),
                                                tally.ctypes.data_as(ctypes.c_void_p), *optrs), name)
        return (status, tally, tuple(outs)) if want_points else (status, tally)

    def keys_check(self, scheme: str, *cols, fmt: str = "affine", want_points: bool = False):
        """`is_valid` of n public keys without verifying anything (`PublicKey::is_valid` & co., and their `from_bytes` with
        `want_points`).  cols: affine / ext (PK[, PK' | Gen]), wire (pk).  Returns (status, tally): status 0 valid, 1 not
        `is_valid`, 3 malformed -- the `key_status` of a key set of these keys; with `want_points` also the tuple of canonical
        affine columns (n, 64), zero rows for malformed items.  Torch CUDA tensors: asynchronous on the current stream;
        numpy arrays: blocking."""
        return self._points_check("keys", scheme, cols, fmt, want_points)

    def signatures_check(self, scheme: str, *cols, fmt: str = "affine", want_points: bool = False):
        """`is_valid` of n signatures (`Signature::is_valid` & co.): cols affine / ext (u, R[, R']), wire (sig).  As
        `keys_check`; a scalar u >= r is malformed.  With `want_points` the third value is (u, R[, R']): the scalar copied and
        the canonical affine points."""
        return self._points_check("signatures", scheme, cols, fmt, want_points)

    _DIGEST_FORMATS = {"canonical": (0, 32), "wide": (1, 64)}

    def digest(self, inputs, lengths=None, *, truncated: bool = False, fmt: str = "canonical"):
        """`Hash::digest(Domain::Other, &item)[0]` of n items (`digest_truncated` with `truncated`): jjs_digest(_dev).  fmt:
        "canonical", elements of 32 bytes little endian below q, or "wide", elements of 64 bytes reduced mod q
        (`BlsScalar::from_bytes_wide`).  inputs: the elements of every item back to back, (n_el, w); `lengths` is then the length
        of every item (an int) or one length per item (a sequence: a ragged call).  With lengths=None the inputs are (n, k, w): n
        items of k elements.  Returns (digests (n, 32), status (n,)): status 3 and a zero row for an item with a canonical element
        >= q, else 0.  The digests are the `m` column of every verify, sign and multisig call.  Torch CUDA tensors: asynchronous
        on the current stream; numpy arrays or bytes: blocking."""
        if fmt not in self._DIGEST_FORMATS:
            raise ValueError(f"fmt {fmt!r}: canonical or wide")
        fid, w = self._DIGEST_FORMATS[fmt]
        dev = _is_torch(inputs)
        if isinstance(inputs, (bytes, bytearray, memoryview)):
            inputs = np.frombuffer(inputs, np.uint8).reshape(-1, w)
        if not dev:
            inputs = np.ascontiguousarray(inputs, dtype=np.uint8)
        offsets, k = None, 0
        if lengths is None:
            if len(inputs.shape) != 3 or inputs.shape[2] != w:
                raise ValueError(f"expected shape (n, k, {w}) when lengths is None, got {tuple(inputs.shape)}")
            n, k = int(inputs.shape[0]), int(inputs.shape[1])
        else:
            if len(inputs.shape) != 2 or inputs.shape[1] != w:
                raise ValueError(f"expected shape (n_el, {w}), got {tuple(inputs.shape)}")
            if np.ndim(lengths) == 0:
                k = int(lengths)
                if k < 1 or inputs.shape[0] % k:
                    raise ValueError(f"{inputs.shape[0]} elements are no whole number of items of {k}")
                n = int(inputs.shape[0]) // k
            else:
                lens = np.asarray(lengths, dtype=np.int64)
                n = len(lens)
                if n and (lens.min() < 1 or int(lens.sum()) != inputs.shape[0] or int(lens.sum()) >= 2**32):
                    raise ValueError("lengths: at least 1 each, and their sum the number of elements")
                offsets = np.zeros(n + 1, np.uint32)
                np.cumsum(lens, out=offsets[1:], dtype=np.uint32)
        off_p = offsets.ctypes.data_as(ctypes.c_void_p) if offsets is not None else None
        flags = 1 if truncated else 0
        if not dev:
            out, status = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
            _ffi.check(self._lib.jjs_digest(fid, flags, inputs.ctypes.data_as(ctypes.c_void_p), off_p, k, n,
                                            out.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p)), "jjs_digest")
            return out, status
        import torch
        if not (inputs.is_cuda and inputs.dtype == torch.uint8 and inputs.is_contiguous()):
            raise ValueError("expected a contiguous uint8 CUDA tensor")
        out = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=inputs.device)[:n]
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=inputs.device)[:n]
        _ffi.check(self._lib.jjs_digest_dev(fid, flags, ctypes.c_void_p(inputs.data_ptr()), off_p, k, n, ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(status.data_ptr()), self._stream()), "jjs_digest_dev")
        return out, status

    def digest_limits(self) -> dict:
        """jjs_debug_digest_limits: the largest n whose items take eight lanes each, and the lanes of the one-lane-per-item
        kernel's grid (a call of more items takes a second trip through it)."""
        out = (ctypes.c_uint64 * 2)()
        _ffi.check(self._lib.jjs_debug_digest_limits(out), "jjs_debug_digest_limits")
        return {"coop_max_items": int(out[0]), "grid_lanes": int(out[1])}

    def verify_wire(self, scheme: str, sig, pk, m, want_status: bool = True):
        """Batch verify from the reference's wire formats (torch CUDA uint8 tensors): sig (n, 64|96|64) =
        u || R [|| R'], pk (n, 32|64|64) compressed, m (n, 32).  Points are decoded on the device; an
        undecodable item gets status 3.  Returns (status, tally), asynchronous on the current stream."""
        ws, wp, wm = self._WIRE_WIDTHS[scheme]
        if not _is_torch(sig):       # numpy: blocking host-buffer call
            hs, hp, hm = self._host(sig, ws), self._host(pk, wp), self._host(m, wm)
            n = hs.shape[0]
            status, tally = np.empty(n, np.uint8), np.zeros(4, np.uint64)
            fn = getattr(self._lib, f"jjs_verify_{scheme}_wire")
            _ffi.check(fn(*[h.ctypes.data_as(ctypes.c_void_p) for h in (hs, hp, hm)], n, status.ctypes.data_as(ctypes.c_void_p),
                          tally.ctypes.data_as(ctypes.c_void_p)), f"jjs_verify_{scheme}_wire")
            return status, tally
        import torch
        n = sig.shape[0]
        ptrs = [self._dev_ptr(sig, ws, n), self._dev_ptr(pk, wp, n), self._dev_ptr(m, wm, n)]
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=sig.device)[:n] if want_status else None
        tally = torch.empty(4, dtype=torch.int64, device=sig.device)
        fn = getattr(self._lib, f"jjs_verify_{scheme}_wire_dev")
        _ffi.check(fn(*ptrs, n, ctypes.c_void_p(status.data_ptr()) if want_status and n else None,
                      ctypes.c_void_p(tally.data_ptr()), self._stream()), f"jjs_verify_{scheme}_wire_dev")
        return status, tally

    def decompress(self, enc):
        """JubJubAffine::from_bytes in bulk: (n, 32) -> ((n, 64) affine, (n,) ok)."""
        import torch
        n = enc.shape[0]
        out = torch.empty((max(n, 1), 64), dtype=torch.uint8, device=enc.device)[:n]
        ok = torch.empty(max(n, 1), dtype=torch.uint8, device=enc.device)[:n]
        _ffi.check(self._lib.jjs_decompress_dev(self._dev_ptr(enc, 32, n), n, ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(ok.data_ptr()), self._stream()), "jjs_decompress_dev")
        return out, ok

    def compress(self, pts):
        """JubJubAffine::to_bytes in bulk: (n, 64) affine -> (n, 32)."""
        import torch
        n = pts.shape[0]
        out = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=pts.device)[:n]
        _ffi.check(self._lib.jjs_compress_dev(self._dev_ptr(pts, 64, n), n, ctypes.c_void_p(out.data_ptr()), self._stream()),
                   "jjs_compress_dev")
        return out

    _MSIG_POINT_WIDTH = {"affine": 64, "ext": 96}

    @classmethod
    def _msig_width(cls, fmt: str) -> int:
        if fmt not in cls._MSIG_POINT_WIDTH:
            raise ValueError(f"the multisignature calls take fmt 'affine' or 'ext', not {fmt!r}")
        return cls._MSIG_POINT_WIDTH[fmt]

    def multisig_combine(self, z, PK, R, S, m, offsets, fmt: str = "affine"):
        """Batch `verify_share` + `combine` + `aggregate_pk` over many transcripts (reference src/multisig.rs).
        z (N, 32), PK / R / S (N, 64) -- or (N, 96) = U || V || Z with fmt="ext", normalised on the device -- m (B, 32);
        offsets: B + 1 ints (host).  torch CUDA uint8 tensors run asynchronously on the current stream
        (jjs_multisig_combine[_ext]_dev), numpy arrays block (jjs_multisig_combine).  Returns
        (share_status (N,), agg_pk (B, 64), sig_u (B, 32), sig_R (B, 64), transcript_status (B,)); statuses 0 ok / 3 / 4;
        sig_u / sig_R are zero for a transcript whose status is not 0 (`combine` returns an error, not a signature)."""
        return self._msig_combine(z, PK, R, S, m, offsets, fmt, False)

    def _msig_combine(self, z, PK, R, S, m, offsets, fmt, _wire):
        """`multisig_combine` (fmt) and `multisig_combine_wire` (_wire: the point columns are (N, 32))."""
        w = 32 if _wire else self._msig_width(fmt)
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
        B, N = len(offs) - 1, z.shape[0]
        if not _is_torch(z):
            hz, hpk, hr, hs, hm = self._host(z, 32), self._host(PK, w), self._host(R, w), self._host(S, w), self._host(m, 32)
            if any(h.shape[0] != N for h in (hpk, hr, hs)) or hm.shape[0] != B or (B and int(offs[-1]) != N):
                raise ValueError("the columns do not have the rows the offsets ask for")
            status, tstatus = np.zeros(N, np.uint8), np.zeros(B, np.uint8)
            agg, su, sr = np.zeros((B, 64), np.uint8), np.zeros((B, 32), np.uint8), np.zeros((B, 64), np.uint8)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            name, head = ("jjs_multisig_combine_wire", []) if _wire else ("jjs_multisig_combine", [self._FORMAT_IDS[fmt]])
            _ffi.check(getattr(self._lib, name)(*head, p(hz), p(hpk), p(hr), p(hs), p(hm), p(offs), B, p(status),
                                                p(tstatus), p(agg), p(su), p(sr)), name)
            return status, agg, su, sr, tstatus
        import torch
        dev_ = z.device
        new = lambda rows, w: torch.empty((max(rows, 1), w), dtype=torch.uint8, device=dev_)[:rows]  # noqa: E731
        status = torch.empty(max(N, 1), dtype=torch.uint8, device=dev_)[:N]
        tstatus = torch.empty(max(B, 1), dtype=torch.uint8, device=dev_)[:B]
        agg, su, sr = new(B, 64), new(B, 32), new(B, 64)
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        name = "jjs_multisig_combine_wire_dev" if _wire else "jjs_multisig_combine_ext_dev" if fmt == "ext" else "jjs_multisig_combine_dev"
        _ffi.check(getattr(self._lib, name)(self._dev_ptr(z, 32, N), self._dev_ptr(PK, w, N), self._dev_ptr(R, w, N),
                                            self._dev_ptr(S, w, N), self._dev_ptr(m, 32, B),
                                            offs.ctypes.data_as(ctypes.c_void_p), B, o(status), o(tstatus), o(agg), o(su),
                                            o(sr), self._stream()), name)
        return status, agg, su, sr, tstatus

    def multisig_combine_wire(self, z, PK_w, R_w, S_w, m, offsets):
        """`multisig_combine` from the reference's wire bytes: PK_w / R_w / S_w (N, 32) = JubJubAffine::to_bytes, decoded on the
        device (jjs_multisig_combine_wire_dev for torch CUDA tensors, the blocking jjs_multisig_combine_wire for numpy arrays).
        The tuple of `multisig_combine` on the decoded columns, byte for byte; a share with an undecodable point gets status 3
        and its transcript no signature.  agg_pk and sig_R are 64-byte affine (`compress` gives their wire bytes)."""
        return self._msig_combine(z, PK_w, R_w, S_w, m, offsets, "affine", True)

    def _msig_verifier(self, handle, keys, offsets, sig, fmt, want_status, _wire: bool = False):
        """The four verifier's calls (include/jjs_gpu.h "verifying aggregate multisignatures"): handle None for inline keys
        (`keys` a PK column in `fmt`), a key-set handle for indices; sig None for aggregation alone, else (u, R, m).  _wire: their
        wire forms ("multisignature from wire encodings"): keys (N, 32), sig = (sig_w (B, 64) = u || R, m)."""
        w = 32 if _wire else self._msig_width(fmt)
        widths = (64, 32) if _wire else (32, w, 32)               # of the columns of `sig`
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
        B, N = len(offs) - 1, keys.shape[0]
        if B and int(offs[-1]) != N:
            raise ValueError("the key column does not have the rows the offsets ask for")
        name = "jjs_multisig_" + ("verify" if sig is not None else "aggregate_pk") + ("_keyset" if handle is not None else "") + \
            ("_wire" if _wire else "")
        head = [] if handle is None else [handle]
        if not _wire and (handle is None or sig is not None):
            head.append(self._FORMAT_IDS[fmt])
        po = offs.ctypes.data_as(ctypes.c_void_p)
        if not _is_torch(keys):
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
            if handle is None:
                hk = self._host(keys, w)
            else:
                hk = np.asarray(keys)
                if hk.dtype.kind not in "iu" or hk.ndim != 1:
                    raise ValueError("key indices must be a 1-d array of integers")
                hk = np.ascontiguousarray(hk, dtype=np.uint32)
            agg = np.zeros((B, 64), np.uint8)
            if sig is None:
                vst = np.zeros(B, np.uint8)
                _ffi.check(getattr(self._lib, name)(*head, p(hk), po, B, p(agg), p(vst)), name)
                return agg, vst
            hsig = [self._host(c, cw) for c, cw in zip(sig, widths)]
            if any(h.shape[0] != B for h in hsig):
                raise ValueError("the signature columns and m take one row per key vector")
            status = np.zeros(B, np.uint8) if want_status else None
            tally = np.zeros(4, np.uint64)
            _ffi.check(getattr(self._lib, name)(*head, p(hk), po, *[p(h) for h in hsig], B, p(agg), p(status), p(tally)), name)
            return status, tally, agg
        import torch
        name += "_dev"
        dev_ = keys.device
        o = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        if handle is None:
            pk = self._dev_ptr(keys, w, N)
        else:
            if not (keys.is_cuda and keys.is_contiguous() and keys.dim() == 1
                    and keys.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("expected a contiguous 1-d CUDA tensor of int32 / uint32 indices, one per key row")
            pk = o(keys)
        agg = torch.empty((max(B, 1), 64), dtype=torch.uint8, device=dev_)[:B]
        if sig is None:
            vst = torch.empty(max(B, 1), dtype=torch.uint8, device=dev_)[:B]
            _ffi.check(getattr(self._lib, name)(*head, pk, po, B, o(agg), o(vst), self._stream()), name)
            return agg, vst
        status = torch.empty(max(B, 1), dtype=torch.uint8, device=dev_)[:B] if want_status else None
        tally = torch.zeros(4, dtype=torch.int64, device=dev_)
        _ffi.check(getattr(self._lib, name)(*head, pk, po, *[self._dev_ptr(c, cw, B) for c, cw in zip(sig, widths)], B, o(agg), o(status),
                                            o(tally), self._stream()), name)
        return status, tally, agg

    def multisig_aggregate_pk_wire(self, PK_w, offsets):
        """`multisig_aggregate_pk` from wire keys: PK_w (N, 32) = PublicKey::to_bytes (jjs_multisig_aggregate_pk_wire[_dev]).
        Returns (agg_pk (B, 64), vec_status (B,)); a vector with an undecodable key gets 3 and a zero aggregate."""
        return self._msig_verifier(None, PK_w, offsets, None, "affine", True, _wire=True)

    def multisig_verify_wire(self, PK_w, offsets, sig_w, m, want_status: bool = True):
        """`multisig_verify` from wire bytes: PK_w (N, 32), sig_w (B, 64) = Signature::to_bytes = u || R, m (B, 32)
        (jjs_multisig_verify_wire[_dev]).  Returns (status, tally, agg_pk): the statuses of `verify_wire("single", ...)` against
        the aggregate, 3 for an undecodable R or an unusable key vector."""
        return self._msig_verifier(None, PK_w, offsets, (sig_w, m), "affine", want_status, _wire=True)

    def multisig_group_wire(self, PK_w) -> "SignerGroup":
        """`multisig_group` from wire keys, (n, 32) = PublicKey::to_bytes (jjs_msig_group_create_wire): the group of the keys they
        decode to; an undecodable key is refused."""
        return SignerGroup(self, PK_w, _wire=True)

    def multisig_aggregate_pk(self, PK, offsets, fmt: str = "affine"):
        """Batch `aggregate_pk` (reference src/multisig.rs:154-156) over many key vectors: PK (N, 64) -- or (N, 96) with
        fmt="ext" -- vector t owning rows offsets[t]:offsets[t+1] (B + 1 host ints).  torch CUDA tensors run asynchronously on
        the current stream (jjs_multisig_aggregate_pk_dev), numpy arrays block (jjs_multisig_aggregate_pk).  Returns
        (agg_pk (B, 64), vec_status (B,)): 0, or 3 and a zero aggregate for a vector with a key that is out of range or off the
        curve; an empty vector gives the identity."""
        return self._msig_verifier(None, PK, offsets, None, fmt, True)

    def multisig_verify(self, PK, offsets, u, R, m, fmt: str = "affine", want_status: bool = True):
        """`aggregate_pk(pk_vec).verify(sig, m)` over many (key vector, signature, message): PK and offsets as in
        `multisig_aggregate_pk`, u (B, 32), R (B, 64) or (B, 96) with fmt="ext", m (B, 32).  Returns (status, tally, agg_pk):
        the statuses of `verify("single", u, R, agg_pk, m)`, 3 and a zero aggregate for an unusable key vector."""
        return self._msig_verifier(None, PK, offsets, (u, R, m), fmt, want_status)

    def multisig_group(self, PK, fmt: str = "affine") -> "SignerGroup":
        """Register the ordered key vector of a committee once (jjs_msig_group_create; fmt="ext": (n, 96) extended keys,
        jjs_msig_group_create_ext): its delinearisation coefficients, its aggregate key and the window tables of its keys are
        built on every driven device and kept until `close()`."""
        return SignerGroup(self, PK, fmt)

    def challenge(self, scheme: str, *arrays):
        """250-bit challenge per item (torch CUDA tensors): single (R, PK, m); double (R, R', PK, PK', m);
        vargen (R, PK, Gen, m)."""
        import torch
        widths = self._WIDTHS[scheme][1:]
        n = arrays[0].shape[0]
        ptrs = [self._dev_ptr(a, w, n) for a, w in zip(arrays, widths)]
        out = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=arrays[0].device)[:n]
        fn = getattr(self._lib, f"jjs_challenge_{scheme}_dev")
        _ffi.check(fn(*ptrs, n, ctypes.c_void_p(out.data_ptr()), self._stream()), f"jjs_challenge_{scheme}_dev")
        return out

    def sign(self, scheme: str, sk, rnd, m, gen_scalar=None):
        """Synthetic-input generator (NOT constant time).  torch CUDA tensors in and out.
        single -> (u, R, PK); double -> (u, R, R', PK, PK'); vargen -> (u, R, PK, Gen)."""
        import torch
        n = sk.shape[0]
        dev = sk.device
        p = lambda t, w=32: self._dev_ptr(t, w, n)  # noqa: E731
        new = lambda w: torch.empty((max(n, 1), w), dtype=torch.uint8, device=dev)[:n]  # noqa: E731
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        u = new(32)
        if scheme == "single":
            R, PK = new(64), new(64)
            _ffi.check(self._lib.jjs_sign_single_dev(p(sk), p(rnd), p(m), n, o(u), o(R), o(PK), self._stream()), "jjs_sign_single_dev")
            return u, R, PK
        if scheme == "double":
            R, Rp, PK, PKp = new(64), new(64), new(64), new(64)
            _ffi.check(self._lib.jjs_sign_double_dev(p(sk), p(rnd), p(m), n, o(u), o(R), o(Rp), o(PK), o(PKp), self._stream()),
                       "jjs_sign_double_dev")
            return u, R, Rp, PK, PKp
        if scheme == "vargen":
            R, PK, Gen = new(64), new(64), new(64)
            _ffi.check(self._lib.jjs_sign_vargen_dev(p(sk), p(gen_scalar), p(rnd), p(m), n, o(u), o(R), o(PK), o(Gen), self._stream()),
                       "jjs_sign_vargen_dev")
            return u, R, PK, Gen
        raise ValueError(scheme)

    def public_keys(self, sk, double: bool = False):
        """`PublicKey::from(&SecretKey)` for a batch (reference src/keys/public.rs:54-60): PK = sk*G, and with
        `double` also PK' = sk*G' (src/keys/public/double.rs:47-57).  torch CUDA tensors; NOT constant time.
        Returns (PK, bad) or (PK, PK', bad); bad[i] = 1 where sk[i] is not a canonical JubJubScalar."""
        import torch
        n = sk.shape[0]
        new = lambda w: torch.empty((max(n, 1), w), dtype=torch.uint8, device=sk.device)[:n]  # noqa: E731
        PK, PKp, bad = new(64), (new(64) if double else None), torch.empty(max(n, 1), dtype=torch.uint8, device=sk.device)[:n]
        o = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and n else None  # noqa: E731
        _ffi.check(self._lib.jjs_public_keys_dev(self._dev_ptr(sk, 32, n), n, o(PK), o(PKp), o(bad), self._stream()),
                   "jjs_public_keys_dev")
        return (PK, PKp, bad) if double else (PK, bad)

    _GEN_WIDTHS = {"affine": 64, "ext": 96, "wire": 32}

    def _vargen_pt(self, sign: bool, sk, Gen, rnd, m, fmt: str):
        w, fmt_id = self._GEN_WIDTHS[fmt], self._FORMAT_IDS[fmt]
        n, ng = sk.shape[0], Gen.shape[0]
        if ng != n and ng != 1:
            raise ValueError(f"Gen has {ng} rows: one per item ({n}) or one for the call")
        if not _is_torch(sk):
            hsk, hgen = self._host(sk, 32), self._host(Gen, w)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
            PK, G_out, status = np.zeros((n, 64), np.uint8), np.zeros((ng, 64), np.uint8), np.zeros(n, np.uint8)
            if not sign:
                _ffi.check(self._lib.jjs_public_keys_vargen(fmt_id, p(hsk), p(hgen), ng, n, p(PK), p(G_out), p(status)), "jjs_public_keys_vargen")
                return PK, G_out, status
            hrnd, hm = self._host(rnd, 32), self._host(m, 32)
            if hrnd.shape[0] != n or hm.shape[0] != n:
                raise ValueError("sk, rnd and m do not have the same rows")
            u, R = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
            _ffi.check(self._lib.jjs_sign_vargen_pt(fmt_id, p(hsk), p(hgen), ng, p(hrnd), p(hm), n, p(u), p(R), p(PK), p(G_out), p(status)),
                       "jjs_sign_vargen_pt")
            return u, R, PK, G_out, status
        import torch
        new = lambda rows, width: torch.empty((max(rows, 1), width), dtype=torch.uint8, device=sk.device)[:rows]  # noqa: E731
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        PK, G_out, status = new(n, 64), new(ng, 64), torch.empty(max(n, 1), dtype=torch.uint8, device=sk.device)[:n]
        if not sign:
            _ffi.check(self._lib.jjs_public_keys_vargen_dev(fmt_id, self._dev_ptr(sk, 32, n), self._dev_ptr(Gen, w, ng), ng, n, o(PK), o(G_out),
                                                            o(status), self._stream()), "jjs_public_keys_vargen_dev")
            return PK, G_out, status
        u, R = new(n, 32), new(n, 64)
        _ffi.check(self._lib.jjs_sign_vargen_pt_dev(fmt_id, self._dev_ptr(sk, 32, n), self._dev_ptr(Gen, w, ng), ng, self._dev_ptr(rnd, 32, n),
                                                    self._dev_ptr(m, 32, n), n, o(u), o(R), o(PK), o(G_out), o(status), self._stream()),
                   "jjs_sign_vargen_pt_dev")
        return u, R, PK, G_out, status

    def public_keys_vargen(self, sk, Gen, fmt: str = "affine"):
        """`PublicKeyVarGen::from(&SecretKeyVarGen)` for a batch with the generator as a POINT: PK = sk * Gen.  sk (n, 32); Gen
        (n, 64) affine, (n, 96) extended or (n, 32) wire by `fmt` -- or ONE row, the generator of the whole call
        (`with_variable_generator` over many keys).  torch CUDA tensors run asynchronously on the current stream
        (jjs_public_keys_vargen_dev), numpy arrays block (jjs_public_keys_vargen).  NOT constant time: test and benchmark
        material.  Returns (PK (n, 64), Gen (rows of Gen, 64) canonical affine, status (n,)): 0, or 3 for sk >= r or an unusable
        generator (a coordinate >= q, Z = 0, an encoding that does not decode, a point off the curve), with zero rows."""
        return self._vargen_pt(False, sk, Gen, None, None, fmt)

    def sign_vargen_pt(self, sk, Gen, rnd, m, fmt: str = "affine"):
        """`SecretKeyVarGen::sign` for a batch given the RNG draws, with the generator as a POINT (any point of the curve: it is
        not validated, as in the reference).  Arguments and dispatch as `public_keys_vargen`, with rnd and m (n, 32).  NOT
        constant time: test and benchmark material.  Returns (u, R, PK, Gen, status); status 3 also for rnd >= r and m >= q."""
        return self._vargen_pt(True, sk, Gen, rnd, m, fmt)

    def sign_limits(self) -> dict:
        """jjs_debug_sign_limits: the lanes of the signing kernels resident at once, and the smallest n from which a signing call
        with one generator takes the shared-generator route (None: no call takes it by size)."""
        out = (ctypes.c_uint64 * 2)()
        _ffi.check(self._lib.jjs_debug_sign_limits(out), "jjs_debug_sign_limits")
        return {"resident_lanes": int(out[0]), "shared_generator_from": None if out[1] == 2**64 - 1 else int(out[1])}

    def _fixed(self, sign: bool, scheme: str, sk, rnd, m, wire: bool):
        if scheme not in ("single", "double"):
            raise ValueError(f"scheme {scheme!r}: single or double (the var-generator scheme signs with sign_vargen_pt)")
        dbl, sid = scheme == "double", self._SCHEME_IDS[scheme]
        nk = sk.shape[0]
        n = rnd.shape[0] if sign else nk
        if nk != n and nk != 1:
            raise ValueError(f"sk has {nk} rows: one per item ({n}) or one for the call")
        # the outputs in the ABI's order: (rows, width), None for what the call does not ask for
        sig = [(n, 32), (n, 64), (n, 64) if dbl else None, (nk, 64), (nk, 64) if dbl else None,
               (n, 96 if dbl else 64) if wire else None, (nk, 64 if dbl else 32) if wire else None]
        shapes = sig if sign else [sig[3], sig[4], sig[6]]
        if not _is_torch(sk):
            hsk = self._host(sk, 32)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
            outs = [np.zeros(s, np.uint8) if s else None for s in shapes]
            status = np.zeros(n, np.uint8)
            if not sign:
                _ffi.check(self._lib.jjs_public_keys_fixed(sid, p(hsk), n, *[p(a) for a in outs], p(status)), "jjs_public_keys_fixed")
            else:
                hrnd, hm = self._host(rnd, 32), self._host(m, 32)
                if hm.shape[0] != n:
                    raise ValueError("rnd and m do not have the same rows")
                _ffi.check(self._lib.jjs_sign_fixed(sid, p(hsk), nk, p(hrnd), p(hm), n, *[p(a) for a in outs], p(status)), "jjs_sign_fixed")
            return tuple(a for a in outs if a is not None) + (status,)
        import torch
        new = lambda s: torch.empty((max(s[0], 1), s[1]), dtype=torch.uint8, device=sk.device)[:s[0]]  # noqa: E731
        o = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and n else None  # noqa: E731
        outs = [new(s) if s else None for s in shapes]
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=sk.device)[:n]
        if not sign:
            _ffi.check(self._lib.jjs_public_keys_fixed_dev(sid, self._dev_ptr(sk, 32, n), n, *[o(t) for t in outs], o(status), self._stream()),
                       "jjs_public_keys_fixed_dev")
        else:
            _ffi.check(self._lib.jjs_sign_fixed_dev(sid, self._dev_ptr(sk, 32, nk), nk, self._dev_ptr(rnd, 32, n), self._dev_ptr(m, 32, n), n,
                                                    *[o(t) for t in outs], o(status), self._stream()), "jjs_sign_fixed_dev")
        return tuple(t for t in outs if t is not None) + (status,)

    def public_keys_fixed(self, scheme: str, sk, wire: bool = False):
        """`PublicKey::from(&SecretKey)` (scheme "single") or `PublicKeyDouble::from(&SecretKey)` ("double") for a batch, with
        range checks and statuses.  sk (n, 32).  torch CUDA tensors run asynchronously on the current stream
        (jjs_public_keys_fixed_dev), numpy arrays block (jjs_public_keys_fixed).  NOT constant time: test and benchmark material.
        Returns (PK[, PK'][, pk_w], status): the affine keys (n, 64), with `wire` also `to_bytes` of them, (n, 32) or (n, 64);
        status (n,) 0, or 3 for sk >= r, with zero rows."""
        return self._fixed(False, scheme, sk, None, None, wire)

    def sign_fixed(self, scheme: str, sk, rnd, m, wire: bool = False):
        """`SecretKey::sign` (scheme "single") or `SecretKey::sign_double` ("double") for a batch given the RNG draws.  rnd and m
        (n, 32); sk (n, 32), or ONE row: the key of the whole call, and then the key outputs have one row.  Dispatch as
        `public_keys_fixed`.  NOT constant time: test and benchmark material.  Returns (u, R[, R'], PK[, PK'][, sig_w, pk_w],
        status): with `wire` also `Signature::to_bytes`, (n, 64) or (n, 96), and the keys' `to_bytes`; status 3 for sk >= r,
        rnd >= r or m >= q, with zero rows."""
        return self._fixed(True, scheme, sk, rnd, m, wire)

    def sign_fixed_limits(self) -> dict:
        """jjs_debug_sign_fixed_limits: the lanes of the SecretKey signing kernels resident at once, and the smallest n from which
        a signing call with one key takes the keyed route (None: no call takes it by size)."""
        out = (ctypes.c_uint64 * 2)()
        _ffi.check(self._lib.jjs_debug_sign_fixed_limits(out), "jjs_debug_sign_fixed_limits")
        return {"resident_lanes": int(out[0]), "keyed_from": None if out[1] == 2**64 - 1 else int(out[1])}

    def multisig_sign_round1(self, r, s):
        """`sign_round_1` for a batch given the two RNG draws (reference src/multisig.rs:169-184): R = r*G, S = s*G.  torch CUDA
        tensors (n, 32); NOT constant time.  Returns (R, S, bad): bad[i] = 1 where r[i] or s[i] is not a canonical
        JubJubScalar, and both rows are then zero."""
        import torch
        n = r.shape[0]
        new = lambda w: torch.empty((max(n, 1), w), dtype=torch.uint8, device=r.device)[:n]  # noqa: E731
        R, S, bad = new(64), new(64), torch.empty(max(n, 1), dtype=torch.uint8, device=r.device)[:n]
        o = lambda t: ctypes.c_void_p(t.data_ptr()) if n else None  # noqa: E731
        _ffi.check(self._lib.jjs_multisig_round1_dev(self._dev_ptr(r, 32, n), self._dev_ptr(s, 32, n), n, o(R), o(S), o(bad), self._stream()),
                   "jjs_multisig_round1_dev")
        return R, S, bad

    def multisig_sign_round2(self, PK, R, S, m, offsets, sk, r, s, signer_row=None, fmt: str = "affine"):
        """`sign_round_2` over many transcripts (reference src/multisig.rs:213-257): a generator of test and benchmark material,
        NOT constant time, and reusing a pair (r, s) is the caller's error.  The transcripts as `multisig_combine` takes them;
        sk, r, s (k, 32) the secrets of the k signing rows; signer_row (k,) the global row each belongs to (None: k == N and
        signing row j is row j).  torch CUDA tensors run asynchronously on the current stream (jjs_multisig_sign_dev), numpy
        arrays block (jjs_multisig_sign).  Returns (z (k, 32), sign_status (k,)): 0, 3 malformed, 5 the transcript does not
        hold this signer at this row exactly once, 7 a duplicated nonce; z is zero behind every status other than 0."""
        w = self._msig_width(fmt)
        fmt_id = self._FORMAT_IDS[fmt]
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
        B, N, k = len(offs) - 1, PK.shape[0], sk.shape[0]
        if (B and int(offs[-1]) != N) or (signer_row is None and k != N) or (signer_row is not None and signer_row.shape[0] != k):
            raise ValueError("the columns do not have the rows the offsets and the signing rows ask for")
        po = offs.ctypes.data_as(ctypes.c_void_p)
        if not _is_torch(PK):
            hpk, hr, hs, hm = self._host(PK, w), self._host(R, w), self._host(S, w), self._host(m, 32)
            hsk, hrr, hss = self._host(sk, 32), self._host(r, 32), self._host(s, 32)
            if any(h.shape[0] != N for h in (hr, hs)) or hm.shape[0] != B or any(h.shape[0] != k for h in (hrr, hss)):
                raise ValueError("the columns do not have the rows the offsets and the signing rows ask for")
            rows = np.ascontiguousarray(signer_row, dtype=np.uint32) if signer_row is not None else None
            z, status = np.zeros((k, 32), np.uint8), np.zeros(k, np.uint8)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
            _ffi.check(self._lib.jjs_multisig_sign(fmt_id, p(hpk), p(hr), p(hs), p(hm), po, B, p(rows), p(hsk), p(hrr), p(hss), k, p(z),
                                                   p(status)), "jjs_multisig_sign")
            return z, status
        import torch
        dev_ = PK.device
        rows = None
        if signer_row is not None:
            if not (signer_row.is_cuda and signer_row.is_contiguous() and signer_row.dim() == 1
                    and signer_row.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("expected a contiguous 1-d CUDA tensor of int32 / uint32 rows, one per signing row")
            rows = ctypes.c_void_p(signer_row.data_ptr())
        z = torch.empty((max(k, 1), 32), dtype=torch.uint8, device=dev_)[:k]
        status = torch.empty(max(k, 1), dtype=torch.uint8, device=dev_)[:k]
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _ffi.check(self._lib.jjs_multisig_sign_dev(fmt_id, self._dev_ptr(PK, w, N), self._dev_ptr(R, w, N), self._dev_ptr(S, w, N),
                                                   self._dev_ptr(m, 32, B), po, B, rows, self._dev_ptr(sk, 32, k), self._dev_ptr(r, 32, k),
                                                   self._dev_ptr(s, 32, k), k, o(z), o(status), self._stream()), "jjs_multisig_sign_dev")
        return z, status

    _MSIG_SHARE_WIDTH = {"affine": 64, "ext": 96, "wire": 32}

    def multisig_verify_share(self, PK, R, S, m, offsets, share_transcript, share_slot, z, fmt: str = "affine", want_R: bool = False):
        """`verify_share` for single shares (reference src/multisig.rs:284-309): the transcripts as `multisig_combine` takes
        them -- PK / R / S (N, 64), (N, 96) with fmt="ext" or (N, 32) with fmt="wire", m (B, 32), offsets B + 1 ints (host) -- and
        Q queries: share_transcript (Q,) and share_slot (Q,) uint32 name the transcript and the participant_index inside it, z
        (Q, 32) is the share.  torch CUDA tensors run asynchronously on the current stream (jjs_multisig_verify_share_dev; the
        two index columns int32 / uint32 tensors), numpy arrays block (jjs_multisig_verify_share).  Returns share_status (Q,):
        0 ok, 3 malformed (the transcript index, z, or an encoding of the transcript), 5 no such participant, 4 the share does
        not verify; with want_R, (share_status, sig_R (B, 64)): the aggregate commitment of every transcript, zero where the
        transcript is malformed or empty."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
        return self._msig_verify_share("jjs_multisig_verify_share", [], PK, None, R, S, m, offs, len(offs) - 1, PK.shape[0],
                                       share_transcript, share_slot, z, fmt, want_R)

    def _msig_verify_share(self, name, head, keys, idx_keys, R, S, m, offs, B, N, qt, qs, z, fmt, want_R):
        """The three verify_share calls: `keys` is the PK column (idx_keys None), a key-set's indices (idx_keys True) or None
        (a signer group, offs None)."""
        if fmt not in self._MSIG_SHARE_WIDTH:
            raise ValueError(f"verify_share takes fmt 'affine', 'ext' or 'wire', not {fmt!r}")
        w, fmt_id = self._MSIG_SHARE_WIDTH[fmt], self._FORMAT_IDS[fmt]
        Q = z.shape[0]
        if offs is not None and B and int(offs[-1]) != N:
            raise ValueError("the columns do not have the rows the offsets ask for")
        po = [offs.ctypes.data_as(ctypes.c_void_p)] if offs is not None else []
        if not _is_torch(z):
            hr, hs, hm, hz = self._host(R, w), self._host(S, w), self._host(m, 32), self._host(z, 32)
            hk = []
            if keys is not None:
                hk = [np.ascontiguousarray(keys, dtype=np.uint32) if idx_keys else self._host(keys, w)]
            hq = [np.ascontiguousarray(q, dtype=np.uint32) for q in (qt, qs)]
            if any(x.shape[0] != N for x in (hr, hs, *hk)) or hm.shape[0] != B or any(q.shape != (Q,) for q in hq):
                raise ValueError("the columns do not have the rows the transcripts and the queries ask for")
            status = np.zeros(Q, np.uint8)
            sr = np.zeros((B, 64), np.uint8) if want_R else None
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
            _ffi.check(getattr(self._lib, name)(*head, fmt_id, *(p(k) for k in hk), p(hr), p(hs), p(hm), *po, B, p(hq[0]), p(hq[1]), p(hz), Q,
                                                p(status), p(sr)), name)
            return (status, sr) if want_R else status
        import torch
        for q in (qt, qs):
            if not (_is_torch(q) and q.is_cuda and q.is_contiguous() and q.shape == (Q,)
                    and q.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("expected contiguous 1-d CUDA tensors of int32 / uint32, one entry per query")
        dev_ = z.device
        status = torch.empty(max(Q, 1), dtype=torch.uint8, device=dev_)[:Q]
        sr = torch.empty((max(B, 1), 64), dtype=torch.uint8, device=dev_)[:B] if want_R else None
        o = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        d = self._dev_ptr
        dk = []
        if keys is not None:
            if idx_keys and not (_is_torch(keys) and keys.is_cuda and keys.is_contiguous() and keys.shape == (N,)
                                 and keys.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("expected a contiguous 1-d CUDA tensor of int32 / uint32 indices, one per participant row")
            dk = [o(keys) if idx_keys else d(keys, w, N)]
        _ffi.check(getattr(self._lib, name + "_dev")(*head, fmt_id, *dk, d(R, w, N), d(S, w, N), d(m, 32, B), *po, B, o(qt), o(qs),
                                                     d(z, 32, Q), Q, o(status), o(sr), self._stream()), name + "_dev")
        return (status, sr) if want_R else status

    # ---- primitives for parity tests ------------------------------------------------------------
    def debug_fq_mul(self, a, b):
        import torch
        n = a.shape[0]
        out = torch.empty_like(a)
        _ffi.check(self._lib.jjs_debug_fq_mul_dev(self._dev_ptr(a, 32, n), self._dev_ptr(b, 32, n), n,
                                                  ctypes.c_void_p(out.data_ptr()), self._stream()), "jjs_debug_fq_mul_dev")
        return out

    def debug_poseidon(self, x):
        import torch
        n, k, w = x.shape
        assert w == 32 and x.is_contiguous()
        out = torch.empty((n, 32), dtype=torch.uint8, device=x.device)
        _ffi.check(self._lib.jjs_debug_poseidon_dev(ctypes.c_void_p(x.data_ptr()), k, n, ctypes.c_void_p(out.data_ptr()),
                                                    self._stream()), "jjs_debug_poseidon_dev")
        return out

    def debug_point_flags(self, pts):
        import torch
        n = pts.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=pts.device)
        _ffi.check(self._lib.jjs_debug_point_flags_dev(self._dev_ptr(pts, 64, n), n, ctypes.c_void_p(out.data_ptr()),
                                                       self._stream()), "jjs_debug_point_flags_dev")
        return out

    def debug_half_scalars(self, c):
        """(a, |b|, sign of b) the device derives from challenges c (n, 32): (n, 16), (n, 16), (n,) uint8 tensors."""
        import torch
        n = c.shape[0]
        a = torch.empty((max(n, 1), 16), dtype=torch.uint8, device=c.device)[:n]
        b = torch.empty((max(n, 1), 16), dtype=torch.uint8, device=c.device)[:n]
        neg = torch.empty(max(n, 1), dtype=torch.uint8, device=c.device)[:n]
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _ffi.check(self._lib.jjs_debug_half_scalars_dev(self._dev_ptr(c, 32, n), n, o(a), o(b), o(neg), self._stream()),
                   "jjs_debug_half_scalars_dev")
        return a, b, neg

    def debug_comb_table(self, which: int) -> np.ndarray:
        nbytes = self._lib.jjs_debug_comb_table_bytes()
        out = np.empty(nbytes // 4, np.uint32)
        _ffi.check(self._lib.jjs_debug_comb_table(which, out.ctypes.data_as(ctypes.c_void_p)), "jjs_debug_comb_table")
        bits = 16 if nbytes == 16 * 65536 * 112 else 8          # digits of the fixed-base comb (csrc/verify_core.h)
        return out.reshape(256 // bits, 1 << bits, 28)

    def debug_dlog_tables(self):
        """The engine's square-root tables (csrc/decode.h): powers (7, 256, 9) uint32 in Montgomery form, logarithms (65536,) uint8."""
        pw, hs = np.empty((7, 256, 9), np.uint32), np.empty(65536, np.uint8)
        _ffi.check(self._lib.jjs_debug_dlog_tables(pw.ctypes.data_as(ctypes.c_void_p), hs.ctypes.data_as(ctypes.c_void_p)),
                   "jjs_debug_dlog_tables")
        return pw, hs

    def sync(self):
        _ffi.check(self._lib.jjs_stream_sync(self._stream()), "jjs_stream_sync")


_engine = None


def engine(device_count: int = 1) -> Engine:
    global _engine
    if _engine is None:
        _engine = Engine(device_count)
    return _engine


# ------------------------------------------------------------------------------------------------
# reference-shaped types: affine points as 64 bytes, scalars as 32 bytes
# ------------------------------------------------------------------------------------------------
def _b(x, n):
    x = bytes(x)
    if len(x) != n:
        raise ValueError(f"expected {n} bytes, got {len(x)}")
    return x


@dataclass(frozen=True)
class Signature:
    """`Signature { u, R }` (reference src/signatures.rs:62-65); R as affine u || v."""
    u: bytes
    R: bytes

    def is_valid(self) -> bool:
        """`Signature::is_valid`: every point on the curve, not the identity and torsion-free."""
        return bool(self.is_valid_batch([self])[0])

    @staticmethod
    def is_valid_batch(items: Sequence) -> np.ndarray:
        """One bool per item (jjs_signatures_check); a malformed encoding is not valid."""
        if not items:
            return np.zeros(0, bool)
        st, _ = engine().signatures_check("single", _rows([s.u for s in items], 32), _rows([s.R for s in items], 64))
        return st == 0


@dataclass(frozen=True)
class SignatureDouble:
    """`SignatureDouble { u, R, R_prime }` (reference src/signatures/double.rs:66-70)."""
    u: bytes
    R: bytes
    R_prime: bytes

    def is_valid(self) -> bool:
        """`SignatureDouble::is_valid`: every point on the curve, not the identity and torsion-free."""
        return bool(self.is_valid_batch([self])[0])

    @staticmethod
    def is_valid_batch(items: Sequence) -> np.ndarray:
        """One bool per item (jjs_signatures_check); a malformed encoding is not valid."""
        if not items:
            return np.zeros(0, bool)
        st, _ = engine().signatures_check("double", _rows([s.u for s in items], 32), _rows([s.R for s in items], 64),
                                        _rows([s.R_prime for s in items], 64))
        return st == 0


@dataclass(frozen=True)
class SignatureVarGen:
    """`SignatureVarGen { u, R }` (reference src/signatures/var_gen.rs)."""
    u: bytes
    R: bytes

    def is_valid(self) -> bool:
        """`SignatureVarGen::is_valid`: every point on the curve, not the identity and torsion-free."""
        return bool(self.is_valid_batch([self])[0])

    @staticmethod
    def is_valid_batch(items: Sequence) -> np.ndarray:
        """One bool per item (jjs_signatures_check); a malformed encoding is not valid."""
        if not items:
            return np.zeros(0, bool)
        st, _ = engine().signatures_check("vargen", _rows([s.u for s in items], 32), _rows([s.R for s in items], 64))
        return st == 0


def _rows(items, width):
    return np.frombuffer(b"".join(_b(x, width) for x in items), np.uint8).reshape(len(items), width)


def _raise_first(status):
    for s in status:
        if s:
            raise _ERRORS[int(s)]()


@dataclass(frozen=True)
class PublicKey:
    """`PublicKey(JubJubExtended)` (reference src/keys/public.rs:52); the point as affine u || v."""
    point: bytes

    def is_valid(self) -> bool:
        """`PublicKey::is_valid`: every point on the curve, not the identity and torsion-free."""
        return bool(self.is_valid_batch([self])[0])

    @staticmethod
    def is_valid_batch(items: Sequence) -> np.ndarray:
        """One bool per key (jjs_keys_check); a malformed encoding is not valid."""
        if not items:
            return np.zeros(0, bool)
        st, _ = engine().keys_check("single", _rows([k.point for k in items], 64))
        return st == 0

    def verify(self, sig: Signature, message: bytes) -> None:
        """`PublicKey::verify` (reference src/keys/public.rs:114-135): returns None or raises."""
        _raise_first(self.verify_batch([(self, sig, message)]))

    @staticmethod
    def verify_batch(items: Sequence[tuple]) -> np.ndarray:
        """items: (PublicKey, Signature, message bytes).  Returns the status byte per item."""
        if not items:
            return np.zeros(0, np.uint8)
        st, _ = engine().verify("single", _rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64),
                                _rows([k.point for k, _, _ in items], 64), _rows([m for _, _, m in items], 32))
        return st

    @staticmethod
    def verify_all(items: Sequence[tuple]) -> bool:
        """items: (PublicKey, Signature, message bytes).  True when every item verifies (one verdict: jjs_verify_all_single)."""
        if not items:
            return True
        ok, _ = engine().verify_all("single", _rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64),
                                    _rows([k.point for k, _, _ in items], 64), _rows([m for _, _, m in items], 32),
                                    statuses_on_failure=False)
        return ok


@dataclass(frozen=True)
class PublicKeyDouble:
    """`PublicKeyDouble(pk, pk_prime)` (reference src/keys/public/double.rs:45)."""
    pk: bytes
    pk_prime: bytes

    def is_valid(self) -> bool:
        """`PublicKeyDouble::is_valid`: every point on the curve, not the identity and torsion-free."""
        return bool(self.is_valid_batch([self])[0])

    @staticmethod
    def is_valid_batch(items: Sequence) -> np.ndarray:
        """One bool per key (jjs_keys_check); a malformed encoding is not valid."""
        if not items:
            return np.zeros(0, bool)
        st, _ = engine().keys_check("double", _rows([k.pk for k in items], 64), _rows([k.pk_prime for k in items], 64))
        return st == 0

    def verify(self, sig: SignatureDouble, message: bytes) -> None:
        """`PublicKeyDouble::verify` (reference src/keys/public/double.rs:86-117)."""
        _raise_first(self.verify_batch([(self, sig, message)]))

    @staticmethod
    def verify_batch(items: Sequence[tuple]) -> np.ndarray:
        if not items:
            return np.zeros(0, np.uint8)
        st, _ = engine().verify(
            "double", _rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64),
            _rows([s.R_prime for _, s, _ in items], 64), _rows([k.pk for k, _, _ in items], 64),
            _rows([k.pk_prime for k, _, _ in items], 64), _rows([m for _, _, m in items], 32))
        return st

    @staticmethod
    def verify_all(items: Sequence[tuple]) -> bool:
        """True when every (PublicKeyDouble, SignatureDouble, message) item verifies (jjs_verify_all_double)."""
        if not items:
            return True
        ok, _ = engine().verify_all(
            "double", _rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64),
            _rows([s.R_prime for _, s, _ in items], 64), _rows([k.pk for k, _, _ in items], 64),
            _rows([k.pk_prime for k, _, _ in items], 64), _rows([m for _, _, m in items], 32), statuses_on_failure=False)
        return ok


@dataclass(frozen=True)
class PublicKeyVarGen:
    """`PublicKeyVarGen { pk, generator }` (reference src/keys/public/var_gen.rs:40-43)."""
    pk: bytes
    generator: bytes

    def is_valid(self) -> bool:
        """`PublicKeyVarGen::is_valid`: every point on the curve, not the identity and torsion-free."""
        return bool(self.is_valid_batch([self])[0])

    @staticmethod
    def is_valid_batch(items: Sequence) -> np.ndarray:
        """One bool per key (jjs_keys_check); a malformed encoding is not valid."""
        if not items:
            return np.zeros(0, bool)
        st, _ = engine().keys_check("vargen", _rows([k.pk for k in items], 64), _rows([k.generator for k in items], 64))
        return st == 0

    def verify(self, sig: SignatureVarGen, message: bytes) -> None:
        """`PublicKeyVarGen::verify` (reference src/keys/public/var_gen.rs:107-133)."""
        _raise_first(self.verify_batch([(self, sig, message)]))

    @staticmethod
    def verify_batch(items: Sequence[tuple]) -> np.ndarray:
        if not items:
            return np.zeros(0, np.uint8)
        st, _ = engine().verify(
            "vargen", _rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64),
            _rows([k.pk for k, _, _ in items], 64), _rows([k.generator for k, _, _ in items], 64),
            _rows([m for _, _, m in items], 32))
        return st

    @staticmethod
    def verify_all(items: Sequence[tuple]) -> bool:
        """True when every (PublicKeyVarGen, SignatureVarGen, message) item verifies (jjs_verify_all_vargen)."""
        if not items:
            return True
        ok, _ = engine().verify_all(
            "vargen", _rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64),
            _rows([k.pk for k, _, _ in items], 64), _rows([k.generator for k, _, _ in items], 64),
            _rows([m for _, _, m in items], 32), statuses_on_failure=False)
        return ok


@dataclass(frozen=True)
class SecretKeyVarGen:
    """`SecretKeyVarGen { sk, generator }` (reference src/keys/secret/var_gen.rs:98-101) with the generator as a POINT: affine
    u || v (64 bytes, `new`) or the 32 bytes of `JubJubAffine::to_bytes` (`from_bytes`, which goes to the device as it is).
    Signing here is a generator of test and benchmark material, NOT constant time: never use with production keys."""
    sk: bytes
    generator: bytes
    fmt: str = "affine"

    @staticmethod
    def new(sk: bytes, generator: bytes) -> "SecretKeyVarGen":
        """`SecretKeyVarGen::new(sk, generator)` (:147): sk 32 bytes, generator affine u || v."""
        return SecretKeyVarGen(_b(sk, 32), _b(generator, 64), "affine")

    @staticmethod
    def from_bytes(data: bytes) -> "SecretKeyVarGen":
        """`SecretKeyVarGen::from_bytes` (:109-131): 64 bytes = sk || generator compressed.  Nothing is decoded here: an
        encoding that does not decode raises `Malformed` when the key is used."""
        data = _b(data, 64)
        return SecretKeyVarGen(data[:32], data[32:], "wire")

    def to_bytes(self) -> bytes:
        """sk || generator compressed (v with the sign of u in the top bit)."""
        if self.fmt == "wire":
            return self.sk + self.generator
        enc = bytearray(self.generator[32:])
        enc[31] |= (self.generator[0] & 1) << 7
        return self.sk + bytes(enc)

    def public_key(self) -> "PublicKeyVarGen":
        """`PublicKeyVarGen::from(&SecretKeyVarGen)`: pk = sk * generator (jjs_public_keys_vargen)."""
        PK, Gen, st = engine().public_keys_vargen(_rows([self.sk], 32), _rows([self.generator], len(self.generator)), fmt=self.fmt)
        _raise_first(st)
        return PublicKeyVarGen(PK[0].tobytes(), Gen[0].tobytes())

    def sign(self, rnd: bytes, message: bytes) -> "SignatureVarGen":
        """`SecretKeyVarGen::sign` (:228-256) given the RNG draw `rnd` the hedged nonce mixes in (32 bytes, < r)."""
        return self.sign_batch([(self, rnd, message)])[0]

    @staticmethod
    def sign_batch(items: Sequence[tuple]) -> list:
        """items: (SecretKeyVarGen, rnd bytes, message bytes).  One SignatureVarGen per item (jjs_sign_vargen_pt, one call per
        generator format among the items); raises `Malformed` for the first item the engine refuses."""
        out = [None] * len(items)
        for fmt in ("affine", "wire"):
            idx = [i for i, (k, _, _) in enumerate(items) if k.fmt == fmt]
            if not idx:
                continue
            u, R, _, _, st = engine().sign_vargen_pt(_rows([items[i][0].sk for i in idx], 32),
                                                     _rows([items[i][0].generator for i in idx], Engine._GEN_WIDTHS[fmt]),
                                                     _rows([items[i][1] for i in idx], 32), _rows([items[i][2] for i in idx], 32), fmt=fmt)
            _raise_first(st)
            for j, i in enumerate(idx):
                out[i] = SignatureVarGen(u[j].tobytes(), R[j].tobytes())
        if any(x is None for x in out):
            raise ValueError("a key's generator format is neither affine nor wire")
        return out


_R_ORDER = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7    # the JubJubScalar modulus


@dataclass(frozen=True)
class SecretKey:
    """`SecretKey(JubJubScalar)` (reference src/keys/secret.rs): the 32 little-endian bytes of the scalar.  Signing and key
    derivation run on the device (jjs_sign_fixed, jjs_public_keys_fixed) and are a generator of test and benchmark material,
    NOT constant time: never use with production keys."""
    sk: bytes

    @staticmethod
    def from_bytes(data: bytes) -> "SecretKey":
        """`SecretKey::from_bytes` (:120-126): refuses a scalar that is not below the group order with `Malformed` (the
        reference's Error::InvalidData), by an integer compare on the host."""
        data = _b(data, 32)
        if int.from_bytes(data, "little") >= _R_ORDER:
            raise Malformed()
        return SecretKey(data)

    def to_bytes(self) -> bytes:
        return self.sk

    def public_key(self) -> "PublicKey":
        """`PublicKey::from(&SecretKey)`: sk * G."""
        PK, st = engine().public_keys_fixed("single", _rows([self.sk], 32))
        _raise_first(st)
        return PublicKey(PK[0].tobytes())

    def public_key_double(self) -> "PublicKeyDouble":
        """`PublicKeyDouble::from(&SecretKey)`: (sk * G, sk * G')."""
        PK, PKp, st = engine().public_keys_fixed("double", _rows([self.sk], 32))
        _raise_first(st)
        return PublicKeyDouble(PK[0].tobytes(), PKp[0].tobytes())

    def sign(self, rnd: bytes, message: bytes) -> "Signature":
        """`SecretKey::sign` (:174-194) given the RNG draw `rnd` the hedged nonce mixes in (32 bytes, < r)."""
        return self.sign_batch([(self, rnd, message)])[0]

    def sign_double(self, rnd: bytes, message: bytes) -> "SignatureDouble":
        """`SecretKey::sign_double` (src/keys/secret/double.rs:56-85) given the RNG draw."""
        return self.sign_double_batch([(self, rnd, message)])[0]

    @staticmethod
    def _sign_cols(scheme: str, items: Sequence[tuple]):
        keys = [k.sk for k, _, _ in items]
        one = len(items) > 1 and all(k == keys[0] for k in keys)          # every item under the same key: one key for the call
        out = engine().sign_fixed(scheme, _rows(keys[:1] if one else keys, 32), _rows([r for _, r, _ in items], 32),
                                  _rows([m for _, _, m in items], 32))
        _raise_first(out[-1])
        return out

    @staticmethod
    def sign_batch(items: Sequence[tuple]) -> list:
        """items: (SecretKey, rnd bytes, message bytes).  One Signature per item from ONE call (jjs_sign_fixed; with one key for
        the call when every item holds the same key); raises `Malformed` for the first item the engine refuses."""
        if not items:
            return []
        u, R = SecretKey._sign_cols("single", items)[:2]
        return [Signature(u[i].tobytes(), R[i].tobytes()) for i in range(len(items))]

    @staticmethod
    def sign_double_batch(items: Sequence[tuple]) -> list:
        """The same for `sign_double`: one SignatureDouble per item."""
        if not items:
            return []
        u, R, Rp = SecretKey._sign_cols("double", items)[:3]
        return [SignatureDouble(u[i].tobytes(), R[i].tobytes(), Rp[i].tobytes()) for i in range(len(items))]

    def with_variable_generator(self, generator: bytes) -> "SecretKeyVarGen":
        """`SecretKey::with_variable_generator` (src/keys/secret/var_gen.rs:34-41): this scalar under `generator`, affine u || v."""
        return SecretKeyVarGen.new(self.sk, generator)


# ------------------------------------------------------------------------------------------------
# registered key sets (include/jjs_gpu.h jjs_keyset_*)
# ------------------------------------------------------------------------------------------------
class KeySet:
    """Keys registered once, verified against by index (`verify`) or by key (`find`, `verify_keys`: the set looks the keys
    up on the device) (`Engine.keyset`).  `key_status[k]`: 0 valid, 1 not `is_valid`, 3 malformed.  Usable as a context
    manager; `close()` destroys the set (queued device calls still complete)."""
    INFO_NAMES = ("scheme", "keys", "valid_keys", "window_bits", "device_bytes", "small_calls", "large_calls")
    _SIG_WIDTHS = {  # (s0, s1, s2) per format; 0: the column is not used
        ("single", "affine"): (32, 64, 0), ("double", "affine"): (32, 64, 64), ("vargen", "affine"): (32, 64, 0),
        ("single", "ext"): (32, 96, 0), ("double", "ext"): (32, 96, 96), ("vargen", "ext"): (32, 96, 0),
        ("single", "wire"): (64, 0, 0), ("double", "wire"): (96, 0, 0), ("vargen", "wire"): (64, 0, 0),
    }

    def __init__(self, eng: Engine, scheme: str, keys, keys2=None, fmt: str = "affine"):
        self._eng, self._lib, self.scheme = eng, eng._lib, scheme
        two = scheme != "single"
        if fmt == "wire":
            if keys2 is not None:
                raise ValueError("wire keys come in one column (pk || pk' or pk || generator): keys2 must be None")
            k1, k2 = eng._host(keys, 64 if two else 32), None
        else:
            w = 96 if fmt == "ext" else 64
            k1 = eng._host(keys, w)
            k2 = eng._host(keys2, w) if two else None
            if two and k2.shape[0] != k1.shape[0]:
                raise ValueError("both key columns must have the same number of keys")
        n = k1.shape[0]
        self.key_status = np.zeros(n, np.uint8)
        h = ctypes.c_uint64(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        _ffi.check(self._lib.jjs_keyset_create(Engine._SCHEME_IDS[scheme], Engine._FORMAT_IDS[fmt], p(k1), p(k2), n,
                                                p(self.key_status), ctypes.byref(h)), "jjs_keyset_create")
        self.handle = h.value
        self.n_keys = n

    @classmethod
    def from_public_keys(cls, keys: Sequence) -> "KeySet":
        """A set of reference-shaped keys, all `PublicKey`, all `PublicKeyDouble` or all `PublicKeyVarGen`."""
        if not keys:
            raise ValueError("a key set needs at least one key")
        if all(isinstance(k, PublicKey) for k in keys):
            return engine().keyset("single", _rows([k.point for k in keys], 64))
        if all(isinstance(k, PublicKeyDouble) for k in keys):
            return engine().keyset("double", _rows([k.pk for k in keys], 64), _rows([k.pk_prime for k in keys], 64))
        if all(isinstance(k, PublicKeyVarGen) for k in keys):
            return engine().keyset("vargen", _rows([k.pk for k in keys], 64), _rows([k.generator for k in keys], 64))
        raise TypeError("keys must all be PublicKey, all PublicKeyDouble or all PublicKeyVarGen")

    def verify_batch(self, items: Sequence[tuple]) -> np.ndarray:
        """items: (key index, Signature | SignatureDouble | SignatureVarGen, message bytes).  Status byte per item."""
        if not items:
            return np.zeros(0, np.uint8)
        idx = np.array([i for i, _, _ in items], np.uint32)
        cols = [_rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64)]
        if self.scheme == "double":
            cols.append(_rows([s.R_prime for _, s, _ in items], 64))
        st, _ = self.verify(idx, *cols, _rows([m for _, _, m in items], 32))
        return st

    def verify(self, idx, *cols, fmt: str = "affine", want_status: bool = True):
        """Verify against the set: `idx` (n,) uint32 key indices, then the signature columns of `fmt` and the messages:
        affine (u, R[, R'], m), ext (u, R_ext[, R'_ext], m), wire (sig, m).  Torch CUDA tensors run asynchronously on the
        current stream (idx an int32 / uint32-sized tensor); numpy arrays block.  Returns (status, tally)."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        widths = [w for w in self._SIG_WIDTHS[(self.scheme, fmt)] if w] + [32]
        if len(cols) != len(widths):
            raise ValueError(f"{self.scheme} {fmt} keyset verify takes {len(widths)} columns after the indices")
        fmt_id = Engine._FORMAT_IDS[fmt]
        slots = [None, None, None, None]          # s0, s1, s2, m
        positions = [0, 1, 2][:len(widths) - 1] + [3]
        if _is_torch(idx):
            import torch
            n = idx.shape[0]
            if not (idx.is_cuda and idx.is_contiguous() and idx.dim() == 1 and idx.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("expected a contiguous 1-d CUDA tensor of int32 / uint32 indices")
            for pos, c, w in zip(positions, cols, widths):
                slots[pos] = self._eng._dev_ptr(c, w, n)
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=idx.device)[:n] if want_status else None
            tally = torch.empty(4, dtype=torch.int64, device=idx.device)
            _ffi.check(self._lib.jjs_keyset_verify_dev(self.handle, fmt_id, ctypes.c_void_p(idx.data_ptr()), *slots, n,
                                                       ctypes.c_void_p(status.data_ptr()) if want_status and n else None,
                                                       ctypes.c_void_p(tally.data_ptr()), self._eng._stream()),
                       "jjs_keyset_verify_dev")
            return status, tally
        hidx = np.asarray(idx)
        if hidx.dtype.kind not in "iu":
            raise ValueError("key indices must be integers")
        hidx = np.ascontiguousarray(hidx, dtype=np.uint32)
        n = hidx.shape[0]
        host = [self._eng._host(c, w) for c, w in zip(cols, widths)]
        if any(h.shape[0] != n for h in host):
            raise ValueError("all columns must have the same number of items as idx")
        for pos, h in zip(positions, host):
            slots[pos] = h.ctypes.data_as(ctypes.c_void_p)
        status, tally = np.empty(n, np.uint8), np.zeros(4, np.uint64)
        _ffi.check(self._lib.jjs_keyset_verify(self.handle, fmt_id, hidx.ctypes.data_as(ctypes.c_void_p), *slots, n,
                                               status.ctypes.data_as(ctypes.c_void_p), tally.ctypes.data_as(ctypes.c_void_p)),
                   "jjs_keyset_verify")
        return status, tally

    # ---- by key (include/jjs_gpu.h "registered key sets by key") ----------------------------------------------
    NOT_IN_SET = 6                   # JJS_STATUS_KEY_NOT_IN_SET
    MISS = 0xFFFFFFFF                # the index `find` reports for a key that is not in the set

    def _key_cols(self, keys, fmt: str):
        """The key columns of the inline call of the set's scheme in `fmt`, as (pointers K0, K1; n; torch?)."""
        two = self.scheme != "single"
        want = 1 if (fmt == "wire" or not two) else 2
        if len(keys) != want:
            raise ValueError(f"{self.scheme} {fmt} keys come in {want} column(s)")
        w = (64 if two else 32) if fmt == "wire" else (96 if fmt == "ext" else 64)
        on_dev = _is_torch(keys[0])
        n = keys[0].shape[0]
        if on_dev:
            ptrs = [self._eng._dev_ptr(k, w, n) for k in keys]
        else:
            host = [self._eng._host(k, w) for k in keys]
            if any(h.shape[0] != n for h in host):
                raise ValueError("both key columns must have the same number of items")
            ptrs = [h.ctypes.data_as(ctypes.c_void_p) for h in host]      # (each keeps its array alive)
        return ptrs + [None] * (2 - len(ptrs)), n, on_dev

    def find(self, *keys, fmt: str = "affine"):
        """The index of every item's key in the set, or `KeySet.MISS`: `keys` are the key columns of the inline call of the
        set's scheme in `fmt` -- affine / ext (PK[, PK' | Gen]), wire (pk).  Torch CUDA tensors run asynchronously on the
        current stream and give an int32 tensor (a miss reads -1); numpy arrays block and give uint32."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        (k0, k1), n, on_dev = self._key_cols(keys, fmt)
        fmt_id = Engine._FORMAT_IDS[fmt]
        if on_dev:
            import torch
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=keys[0].device)[:n]
            _ffi.check(self._lib.jjs_keyset_find_dev(self.handle, fmt_id, k0, k1, n, ctypes.c_void_p(idx.data_ptr()), self._eng._stream()),
                       "jjs_keyset_find_dev")
            return idx
        idx = np.empty(n, np.uint32)
        _ffi.check(self._lib.jjs_keyset_find(self.handle, fmt_id, k0, k1, n, idx.ctypes.data_as(ctypes.c_void_p)), "jjs_keyset_find")
        return idx

    def verify_keys(self, keys, *cols, fmt: str = "affine", want_status: bool = True, want_idx: bool = False):
        """Verify against the set BY KEY: `keys` is the tuple of key columns `find` takes, then the signature columns and the
        messages of `verify`.  Torch CUDA tensors: asynchronous; an item whose key is not in the set gets status
        `KeySet.NOT_IN_SET` and is counted in no tally word.  numpy arrays: blocking, and a drop-in for the inline call --
        such items are verified inline, status and tally are those of `Engine.verify` / `verify_ext` / `verify_wire` on the
        same columns.  Returns (status, tally), and the found indices as a third value with `want_idx`."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        if not isinstance(keys, (tuple, list)):
            keys = (keys,)
        (k0, k1), n, on_dev = self._key_cols(keys, fmt)
        widths = [w for w in self._SIG_WIDTHS[(self.scheme, fmt)] if w] + [32]
        if len(cols) != len(widths):
            raise ValueError(f"{self.scheme} {fmt} keyset verify takes {len(widths)} columns after the keys")
        fmt_id = Engine._FORMAT_IDS[fmt]
        slots = [None, None, None, None]          # s0, s1, s2, m
        positions = [0, 1, 2][:len(widths) - 1] + [3]
        if on_dev:
            import torch
            dev = keys[0].device
            for pos, c, w in zip(positions, cols, widths):
                slots[pos] = self._eng._dev_ptr(c, w, n)
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n] if want_status else None
            tally = torch.empty(4, dtype=torch.int64, device=dev)
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n] if want_idx else None
            _ffi.check(self._lib.jjs_keyset_verify_keys_dev(self.handle, fmt_id, k0, k1, *slots, n,
                                                            ctypes.c_void_p(status.data_ptr()) if want_status and n else None,
                                                            ctypes.c_void_p(tally.data_ptr()),
                                                            ctypes.c_void_p(idx.data_ptr()) if want_idx and n else None, self._eng._stream()),
                       "jjs_keyset_verify_keys_dev")
            return (status, tally, idx) if want_idx else (status, tally)
        host = [self._eng._host(c, w) for c, w in zip(cols, widths)]
        if any(h.shape[0] != n for h in host):
            raise ValueError("all columns must have the same number of items as the keys")
        for pos, h in zip(positions, host):
            slots[pos] = h.ctypes.data_as(ctypes.c_void_p)
        status, tally, idx = np.empty(n, np.uint8), np.zeros(4, np.uint64), np.empty(n, np.uint32)
        _ffi.check(self._lib.jjs_keyset_verify_keys(self.handle, fmt_id, k0, k1, *slots, n, status.ctypes.data_as(ctypes.c_void_p),
                                                    tally.ctypes.data_as(ctypes.c_void_p),
                                                    idx.ctypes.data_as(ctypes.c_void_p) if want_idx else None), "jjs_keyset_verify_keys")
        return (status, tally, idx) if want_idx else (status, tally)

    def verify_all_batch(self, items: Sequence[tuple]) -> bool:
        """items: as for `verify_batch`.  True when every item verifies (one verdict: jjs_keyset_verify_all)."""
        if not items:
            return True
        idx = np.array([i for i, _, _ in items], np.uint32)
        cols = [_rows([s.u for _, s, _ in items], 32), _rows([s.R for _, s, _ in items], 64)]
        if self.scheme == "double":
            cols.append(_rows([s.R_prime for _, s, _ in items], 64))
        ok, _ = self.verify_all(idx, *cols, _rows([m for _, _, m in items], 32), statuses_on_failure=False)
        return ok

    def verify_all(self, idx, *cols, fmt: str = "affine", statuses_on_failure: bool = True):
        """One verdict for the whole batch against the set (jjs_keyset_verify_all): True when every item would get status
        0 from `verify`.  Same arguments as `verify`.  numpy inputs: blocking, returns (bool, status or None) -- the
        statuses of `verify`, byte for byte, when the verdict is False and `statuses_on_failure` is set.  torch CUDA
        tensors: asynchronous on the current stream, returns a device uint32 tensor of one element (1 accepted, 0 not);
        run `verify` for the statuses."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        widths = [w for w in self._SIG_WIDTHS[(self.scheme, fmt)] if w] + [32]
        if len(cols) != len(widths):
            raise ValueError(f"{self.scheme} {fmt} keyset verify_all takes {len(widths)} columns after the indices")
        fmt_id = Engine._FORMAT_IDS[fmt]
        slots = [None, None, None, None]          # s0, s1, s2, m
        positions = [0, 1, 2][:len(widths) - 1] + [3]
        if _is_torch(idx):
            import torch
            n = idx.shape[0]
            if not (idx.is_cuda and idx.is_contiguous() and idx.dim() == 1 and idx.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("expected a contiguous 1-d CUDA tensor of int32 / uint32 indices")
            for pos, c, w in zip(positions, cols, widths):
                slots[pos] = self._eng._dev_ptr(c, w, n)
            verdict = torch.empty(1, dtype=torch.int32, device=idx.device)
            _ffi.check(self._lib.jjs_keyset_verify_all_dev(self.handle, fmt_id, ctypes.c_void_p(idx.data_ptr()), *slots, n,
                                                           ctypes.c_void_p(verdict.data_ptr()), self._eng._stream()),
                       "jjs_keyset_verify_all_dev")
            return verdict.view(torch.uint32) if hasattr(torch, "uint32") else verdict
        hidx = np.asarray(idx)
        if hidx.dtype.kind not in "iu":
            raise ValueError("key indices must be integers")
        hidx = np.ascontiguousarray(hidx, dtype=np.uint32)
        n = hidx.shape[0]
        host = [self._eng._host(c, w) for c, w in zip(cols, widths)]
        if any(h.shape[0] != n for h in host):
            raise ValueError("all columns must have the same number of items as idx")
        for pos, h in zip(positions, host):
            slots[pos] = h.ctypes.data_as(ctypes.c_void_p)
        status = np.empty(n, np.uint8) if statuses_on_failure else None
        verdict = ctypes.c_int(-1)
        _ffi.check(self._lib.jjs_keyset_verify_all(self.handle, fmt_id, hidx.ctypes.data_as(ctypes.c_void_p), *slots, n,
                                                   status.ctypes.data_as(ctypes.c_void_p) if status is not None else None,
                                                   ctypes.byref(verdict)), "jjs_keyset_verify_all")
        ok = verdict.value == 1
        return ok, (None if ok or status is None else status)

    def multisig_combine(self, key_idx, z, R, S, m, offsets, fmt: str = "affine"):
        """`Engine.multisig_combine` for committees drawn from this set (scheme "single"): key_idx (N,) uint32 names the key of
        every share instead of a PK column; z (N, 32), R / S (N, 64) -- or (N, 96) with fmt="ext" -- m (B, 32), offsets B + 1
        ints (host).  torch CUDA tensors run asynchronously on the current stream (jjs_multisig_combine_keyset_dev; key_idx an
        int32 / uint32 tensor), numpy arrays block (jjs_multisig_combine_keyset).  Returns the tuple of
        `Engine.multisig_combine`, byte for byte what it gives with the registered keys in the PK column -- except that a
        transcript naming an index outside the set or a key whose `key_status` is not 0 is refused: status 3 on all its
        shares and on the transcript, agg_pk / sig_u / sig_R zero."""
        return self._msig_combine(key_idx, z, R, S, m, offsets, fmt, False)

    def _msig_combine(self, key_idx, z, R, S, m, offsets, fmt, _wire):
        """`multisig_combine` (fmt) and `multisig_combine_wire` (_wire: R and S are (N, 32))."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        w = 32 if _wire else Engine._msig_width(fmt)
        head = [self.handle] if _wire else [self.handle, Engine._FORMAT_IDS[fmt]]
        name = "jjs_multisig_combine_keyset_wire" if _wire else "jjs_multisig_combine_keyset"
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
        B, N = len(offs) - 1, z.shape[0]
        if not _is_torch(z):
            hidx = np.asarray(key_idx)
            if hidx.dtype.kind not in "iu":
                raise ValueError("key indices must be integers")
            hidx = np.ascontiguousarray(hidx, dtype=np.uint32)
            h = self._eng._host
            hz, hr, hs, hm = h(z, 32), h(R, w), h(S, w), h(m, 32)
            if hidx.shape != (N,) or any(x.shape[0] != N for x in (hr, hs)) or hm.shape[0] != B or (B and int(offs[-1]) != N):
                raise ValueError("the columns do not have the rows the offsets ask for")
            status, tstatus = np.zeros(N, np.uint8), np.zeros(B, np.uint8)
            agg, su, sr = np.zeros((B, 64), np.uint8), np.zeros((B, 32), np.uint8), np.zeros((B, 64), np.uint8)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            _ffi.check(getattr(self._lib, name)(*head, p(hidx), p(hz), p(hr), p(hs), p(hm), p(offs), B, p(status),
                                                p(tstatus), p(agg), p(su), p(sr)), name)
            return status, agg, su, sr, tstatus
        import torch
        if not (_is_torch(key_idx) and key_idx.is_cuda and key_idx.is_contiguous() and key_idx.shape == (N,)
                and key_idx.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
            raise ValueError("expected a contiguous 1-d CUDA tensor of int32 / uint32 indices, one per share")
        dev_ = z.device
        new = lambda rows, w: torch.empty((max(rows, 1), w), dtype=torch.uint8, device=dev_)[:rows]  # noqa: E731
        status = torch.empty(max(N, 1), dtype=torch.uint8, device=dev_)[:N]
        tstatus = torch.empty(max(B, 1), dtype=torch.uint8, device=dev_)[:B]
        agg, su, sr = new(B, 64), new(B, 32), new(B, 64)
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        d = Engine._dev_ptr
        _ffi.check(getattr(self._lib, name + "_dev")(*head, o(key_idx), d(z, 32, N), d(R, w, N), d(S, w, N),
                                                     d(m, 32, B), offs.ctypes.data_as(ctypes.c_void_p), B, o(status), o(tstatus),
                                                     o(agg), o(su), o(sr), Engine._stream()), name + "_dev")
        return status, agg, su, sr, tstatus

    def multisig_combine_wire(self, key_idx, z, R_w, S_w, m, offsets):
        """`multisig_combine` with R_w / S_w (N, 32) in the wire encoding, decoded on the device
        (jjs_multisig_combine_keyset_wire[_dev]); a share with an undecodable point gets status 3."""
        return self._msig_combine(key_idx, z, R_w, S_w, m, offsets, "affine", True)

    def multisig_verify_share(self, key_idx, R, S, m, offsets, share_transcript, share_slot, z, fmt: str = "affine", want_R: bool = False):
        """`Engine.multisig_verify_share` for committees drawn from this set (scheme "single"): key_idx (N,) uint32 names the
        key of every participant row instead of a PK column (jjs_multisig_verify_share_keyset[_dev]).  Every query of a
        transcript naming an index outside the set, or a key the set refused or has removed, gets status 3."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        if not _is_torch(key_idx) and np.asarray(key_idx).dtype.kind not in "iu":
            raise ValueError("key indices must be integers")
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
        return self._eng._msig_verify_share("jjs_multisig_verify_share_keyset", [self.handle], key_idx, True, R, S, m, offs, len(offs) - 1,
                                            R.shape[0], share_transcript, share_slot, z, fmt, want_R)

    def multisig_verify_wire(self, key_idx, offsets, sig_w, m, want_status: bool = True):
        """`multisig_verify` with the aggregate signature as sig_w (B, 64) = u || R (jjs_multisig_verify_keyset_wire[_dev]).
        Returns (status, tally, agg_pk)."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        return self._eng._msig_verifier(self.handle, key_idx, offsets, (sig_w, m), "affine", want_status, _wire=True)

    def multisig_aggregate_pk(self, key_idx, offsets):
        """`Engine.multisig_aggregate_pk` with the keys named by index into this set (scheme "single"): key_idx (N,) uint32.  A
        vector naming an index outside the set or a key whose `key_status` is not 0 is refused (vec_status 3, zero aggregate)."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        return self._eng._msig_verifier(self.handle, key_idx, offsets, None, "affine", True)

    def multisig_verify(self, key_idx, offsets, u, R, m, fmt: str = "affine", want_status: bool = True):
        """`Engine.multisig_verify` with the keys named by index into this set; fmt is that of R.  Returns (status, tally, agg_pk)."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        return self._eng._msig_verifier(self.handle, key_idx, offsets, (u, R, m), fmt, want_status)

    def info(self) -> dict:
        out = (ctypes.c_uint64 * len(self.INFO_NAMES))()
        _ffi.check(self._lib.jjs_keyset_info(self.handle, out), "jjs_keyset_info")
        return dict(zip(self.INFO_NAMES, (int(v) for v in out)))

    # ---- adding keys to the live set (include/jjs_gpu.h "adding keys to a live key set") -----------------------
    GROWTH_NAMES = ("capacity", "add_calls", "relocations", "lookup_rebuilds", "add_known")

    def add(self, keys, keys2=None, fmt: str = "affine", unique: bool = False):
        """Register more keys (`keys`, `keys2`, `fmt` as `Engine.keyset` takes them; numpy, blocking).  Appended, candidate i
        goes to index n_keys + i whatever it is; with `unique` a candidate the set or an earlier candidate already holds gets
        that index, and a malformed one `KeySet.MISS`.  Old indices never change.  Returns (idx, key_status), one entry per
        candidate; `n_keys` and `key_status` follow the set."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        two = self.scheme != "single"
        if fmt == "wire":
            if keys2 is not None:
                raise ValueError("wire keys come in one column (pk || pk' or pk || generator): keys2 must be None")
            k1, k2 = self._eng._host(keys, 64 if two else 32), None
        else:
            w = 96 if fmt == "ext" else 64
            k1 = self._eng._host(keys, w)
            k2 = self._eng._host(keys2, w) if two else None
            if two and k2.shape[0] != k1.shape[0]:
                raise ValueError("both key columns must have the same number of keys")
        n = k1.shape[0]
        idx, status, added = np.empty(n, np.uint32), np.empty(n, np.uint8), ctypes.c_size_t(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        _ffi.check(self._lib.jjs_keyset_add(self.handle, Engine._FORMAT_IDS[fmt], p(k1), p(k2), n, 1 if unique else 0, p(status), p(idx),
                                             ctypes.byref(added)), "jjs_keyset_add")
        grown = np.zeros(self.n_keys + added.value, np.uint8)
        grown[:self.n_keys] = self.key_status
        fresh = (idx != self.MISS) & (idx >= self.n_keys)
        grown[idx[fresh]] = status[fresh]
        self.key_status, self.n_keys = grown, self.n_keys + added.value
        return idx, status

    def reserve(self, n: int) -> None:
        """Room for `n` keys in all: the adds up to there write in place and move nothing."""
        _ffi.check(self._lib.jjs_keyset_reserve(self.handle, n), "jjs_keyset_reserve")

    def growth(self) -> dict:
        out = (ctypes.c_uint64 * len(self.GROWTH_NAMES))()
        _ffi.check(self._lib.jjs_keyset_growth(self.handle, out), "jjs_keyset_growth")
        return dict(zip(self.GROWTH_NAMES, (int(v) for v in out)))

    # ---- removing keys, and compacting the set (include/jjs_gpu.h "removing keys from a live key set") ---------
    REMOVAL_NAMES = ("removed_keys", "live_keys", "remove_calls", "compact_calls")
    WAS_REMOVED, NOT_IN_RANGE = 8, 0xFF

    @property
    def removed(self) -> np.ndarray:
        """Boolean mask over the indices: removed, and not yet dropped by `compact`."""
        mask = getattr(self, "_removed", None)
        if mask is None or len(mask) != self.n_keys:
            grown = np.zeros(self.n_keys, bool)
            if mask is not None:
                grown[:min(len(mask), self.n_keys)] = mask[:self.n_keys]
            self._removed = mask = grown
        return mask

    def remove(self, idx):
        """Remove the keys at `idx` (uint32 indices; numpy, blocking), in place: no index moves, a removed index verifies
        nothing (status 3) and its key is found nowhere.  Returns (result, n_removed): per index the key's status before the
        call (0, 1, 3), `KeySet.WAS_REMOVED` or `KeySet.NOT_IN_RANGE`; and the distinct indices this call removed.
        `key_status` becomes 3 at removed indices."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), np.uint32)
        result, n_removed = np.empty(len(idx), np.uint8), ctypes.c_size_t(0)
        _ffi.check(self._lib.jjs_keyset_remove(self.handle, idx.ctypes.data_as(ctypes.c_void_p), len(idx),
                                                result.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_removed)), "jjs_keyset_remove")
        gone = idx[idx < self.n_keys]
        mask = self.removed
        mask[gone] = True
        self.key_status[gone] = 3
        return result, n_removed.value

    def compact(self) -> np.ndarray:
        """Drop the removed keys: the set becomes `Engine.keyset` of the survivors in their order, in a new allocation (`Engine.trim`
        frees the old one).  EVERY INDEX CHANGES: returns the map, `map[i]` the new index of old index i, `KeySet.MISS` for a
        removed one.  `n_keys`, `key_status` and `removed` follow."""
        if self.handle == 0:
            raise _ffi.JjsError("the key set is closed")
        m, n_new = np.empty(self.n_keys, np.uint32), ctypes.c_size_t(0)
        _ffi.check(self._lib.jjs_keyset_compact(self.handle, m.ctypes.data_as(ctypes.c_void_p), len(m), ctypes.byref(n_new)), "jjs_keyset_compact")
        keep = m != self.MISS
        self.key_status, self.n_keys = np.ascontiguousarray(self.key_status[keep]), n_new.value
        self._removed = np.zeros(self.n_keys, bool)
        return m

    def removal(self) -> dict:
        out = (ctypes.c_uint64 * len(self.REMOVAL_NAMES))()
        _ffi.check(self._lib.jjs_keyset_removal(self.handle, out), "jjs_keyset_removal")
        return dict(zip(self.REMOVAL_NAMES, (int(v) for v in out)))

    def close(self) -> None:
        if self.handle:
            h, self.handle = self.handle, 0
            _ffi.check(self._lib.jjs_keyset_destroy(h), "jjs_keyset_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ------------------------------------------------------------------------------------------------
# multisig signer groups (include/jjs_gpu.h jjs_msig_group_*)
# ------------------------------------------------------------------------------------------------
class SignerGroup:
    """The signers of a multisignature registered once (`Engine.multisig_group`); `combine` then takes transcripts of exactly
    these participants, in this order.  `aggregate_pk`: the 64 bytes of aggregate_pk(pk_vec).  Usable as a context manager;
    `close()` destroys the group (queued device calls still complete)."""
    INFO_NAMES = ("participants", "window_bits", "device_bytes", "calls")

    def __init__(self, eng: Engine, PK, fmt: str = "affine", _wire: bool = False):
        self._eng, self._lib = eng, eng._lib
        pk = eng._host(PK, 32 if _wire else Engine._msig_width(fmt))
        h = ctypes.c_uint64(0)
        name = "jjs_msig_group_create_wire" if _wire else "jjs_msig_group_create_ext" if fmt == "ext" else "jjs_msig_group_create"
        _ffi.check(getattr(self._lib, name)(pk.ctypes.data_as(ctypes.c_void_p) if len(pk) else None, len(pk), ctypes.byref(h)), name)
        self.handle = h.value
        self.participants = len(pk)
        self.aggregate_pk = np.zeros(64, np.uint8)
        _ffi.check(self._lib.jjs_msig_group_aggregate_pk(self.handle, self.aggregate_pk.ctypes.data_as(ctypes.c_void_p)),
                   "jjs_msig_group_aggregate_pk")

    def combine_wire(self, z, R_w, S_w, m):
        """`combine` with R_w / S_w (B n, 32) in the wire encoding, decoded on the device (jjs_msig_group_combine_wire[_dev]); a
        share with an undecodable point gets status 3."""
        return self._combine(z, R_w, S_w, m, "affine", True)

    def combine(self, z, R, S, m, fmt: str = "affine"):
        """Batch `verify_share` + `combine` over B transcripts of the group's n participants: z (B n, 32), R / S (B n, 64) -- or
        (B n, 96) = U || V || Z with fmt="ext" -- m (B, 32), share (t, i) at row t n + i.  torch CUDA uint8 tensors run
        asynchronously on the current stream, numpy arrays block (jjs_msig_group_combine).  Returns (share_status (B n,),
        sig_u (B, 32), sig_R (B, 64), transcript_status (B,)): the tuple of `Engine.multisig_combine` without agg_pk, byte for byte."""
        return self._combine(z, R, S, m, fmt, False)

    def _combine(self, z, R, S, m, fmt, _wire):
        """`combine` (fmt) and `combine_wire` (_wire: R and S are (B n, 32))."""
        w = 32 if _wire else Engine._msig_width(fmt)
        B = m.shape[0]
        N = B * self.participants
        if not _is_torch(z):
            h = self._eng._host
            hz, hr, hs, hm = h(z, 32), h(R, w), h(S, w), h(m, 32)
            if any(x.shape[0] != N for x in (hz, hr, hs)):
                raise ValueError(f"expected {N} rows: {B} transcripts of {self.participants} participants")
            status, tstatus = np.zeros(N, np.uint8), np.zeros(B, np.uint8)
            su, sr = np.zeros((B, 32), np.uint8), np.zeros((B, 64), np.uint8)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            name, head = ("jjs_msig_group_combine_wire", []) if _wire else ("jjs_msig_group_combine", [Engine._FORMAT_IDS[fmt]])
            _ffi.check(getattr(self._lib, name)(self.handle, *head, p(hz), p(hr), p(hs), p(hm), B, p(status),
                                                p(tstatus), p(su), p(sr)), name)
            return status, su, sr, tstatus
        import torch
        dev_ = z.device
        new = lambda rows, w: torch.empty((max(rows, 1), w), dtype=torch.uint8, device=dev_)[:rows]  # noqa: E731
        status = torch.empty(max(N, 1), dtype=torch.uint8, device=dev_)[:N]
        tstatus = torch.empty(max(B, 1), dtype=torch.uint8, device=dev_)[:B]
        su, sr = new(B, 32), new(B, 64)
        o = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        d = Engine._dev_ptr
        name = "jjs_msig_group_combine_wire_dev" if _wire else "jjs_msig_group_combine_ext_dev" if fmt == "ext" else "jjs_msig_group_combine_dev"
        _ffi.check(getattr(self._lib, name)(self.handle, d(z, 32, N), d(R, w, N), d(S, w, N), d(m, 32, B), B, o(status),
                                            o(tstatus), o(su), o(sr), Engine._stream()), name)
        return status, su, sr, tstatus

    def verify_share(self, R, S, m, share_transcript, share_slot, z, fmt: str = "affine", want_R: bool = False):
        """`Engine.multisig_verify_share` over B transcripts of the group's n participants (R / S (B n, ...), m (B, 32), share
        (t, i) at row t n + i): the group's d_i, aggregate key and tables are on the device already
        (jjs_msig_group_verify_share[_dev])."""
        B = m.shape[0]
        return self._eng._msig_verify_share("jjs_msig_group_verify_share", [self.handle], None, None, R, S, m, None, B, B * self.participants,
                                            share_transcript, share_slot, z, fmt, want_R)

    def info(self) -> dict:
        out = (ctypes.c_uint64 * len(self.INFO_NAMES))()
        _ffi.check(self._lib.jjs_msig_group_info(self.handle, out), "jjs_msig_group_info")
        return dict(zip(self.INFO_NAMES, (int(x) for x in out)))

    def close(self) -> None:
        h, self.handle = self.handle, 0
        if h:
            _ffi.check(self._lib.jjs_msig_group_destroy(h), "jjs_msig_group_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

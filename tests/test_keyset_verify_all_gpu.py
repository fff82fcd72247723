"""jjs_keyset_verify_all* on the device: the routed entry points (product library) on valid batches of every scheme, size
band and signature format over a 4 096-key set, the empty batch, one spoilt item per failure class with the statuses of
KeySet.verify and the oracle, a bad index, an invalid registered key, a stale handle and four threads at once; then
keyset_verify_all_child.py forces the verdict algorithm (profiling build)."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from helpers import ARG_ORDER, IDENT, make_batch, oracle_verify
from keyset_verify_all_cases import KEYCOLS, register_cols, sig_cols
from verify_all_cases import device_batch, spoil_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMES = ["single", "double", "vargen"]
FORMATS = ["affine", "ext", "wire"]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_verdict(ks, idx, cols, fmt="affine"):
    import torch
    v = ks.verify_all(dev(idx), *[dev(c) for c in cols], fmt=fmt)
    torch.cuda.synchronize()
    return int(v.cpu().view(torch.int32).item())


def test_the_abi_has_the_entry_points():
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    assert lib.jjs_abi_version() == 5
    assert hasattr(lib, "jjs_keyset_verify_all") and hasattr(lib, "jjs_keyset_verify_all_dev")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_valid_batches_every_size_band_and_format(eng, scheme):
    for n in (1, 65, 16385, 1 << 17):
        cols = [c.cpu().numpy() for c in device_batch(eng, scheme, n, 4096)]
        b = dict(zip(ARG_ORDER[scheme], cols))
        nk = min(n, 4096)
        idx = (np.arange(n) % nk).astype(np.uint32)
        with eng.keyset(scheme, *[b[k][:nk] for k in KEYCOLS[scheme]]) as ks:
            assert (ks.key_status == 0).all()
            for fmt in FORMATS:
                sigs = sig_cols(eng, scheme, b, fmt)
                assert dev_verdict(ks, idx, sigs, fmt) == 1, (n, fmt)
                assert ks.verify_all(idx, *sigs, fmt=fmt) == (True, None), (n, fmt)
            info = ks.info()           # the product routes every call to the per-item route, which counts as KeySet.verify does
            assert info["small_calls" if n <= 16384 else "large_calls"] == 6 and info["large_calls" if n <= 16384 else "small_calls"] == 0


@pytest.mark.parametrize("scheme", SCHEMES)
def test_empty_batch_is_accepted(eng, scheme):
    b = make_batch(scheme, 4, seed=3, n_keys=4, mix=False)
    keys, _ = register_cols(scheme, b)
    with eng.keyset(scheme, *keys) as ks:
        for fmt in FORMATS:
            sigs = [c[:0] for c in sig_cols(eng, scheme, b, fmt)]
            assert ks.verify_all(np.zeros(0, np.uint32), *sigs, fmt=fmt) == (True, None)
            assert dev_verdict(ks, np.zeros(0, np.uint32), sigs, fmt) == 1
        assert ks.verify_all_batch([]) is True


def _check_rejected(eng, ks, scheme, b, idx, want, name):
    for fmt in FORMATS:
        if fmt == "wire" and name.startswith("noncanonical"):
            continue                                  # a coordinate >= q has no compressed encoding
        sigs = sig_cols(eng, scheme, b, fmt)
        ok, st = ks.verify_all(idx, *sigs, fmt=fmt)
        per_item, _ = ks.verify(idx, *sigs, fmt=fmt)
        assert not ok, (name, fmt)
        assert st.tolist() == per_item.tolist() == want.tolist(), (name, fmt)
        assert dev_verdict(ks, idx, sigs, fmt) == 0, (name, fmt)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_spoilt_item_statuses_match_keyset_verify(eng, scheme):
    base = make_batch(scheme, 65, seed=41, n_keys=16, mix=False)
    for name, b in spoil_cases(scheme, base):
        keys, idx = register_cols(scheme, b)            # a spoilt key is a registered (invalid) key
        want = oracle_verify(scheme, b)
        assert (want != 0).sum() == 1, name
        with eng.keyset(scheme, *keys) as ks:
            _check_rejected(eng, ks, scheme, b, idx, want, name)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_bad_index_and_invalid_registered_key(eng, scheme):
    b = make_batch(scheme, 65, seed=43, n_keys=8, mix=False)
    keys, idx = register_cols(scheme, b)
    ident = keys[0][:1].copy(); ident[0] = IDENT
    keys = [np.concatenate([k, ident]) if i == 0 else np.concatenate([k, k[:1]]) for i, k in enumerate(keys)]
    with eng.keyset(scheme, *keys) as ks:
        assert ks.key_status[-1] == 1
        assert ks.verify_all(idx, *sig_cols(eng, scheme, b, "affine")) == (True, None)
        for bad, status in ((len(keys[0]), 3), (0xFFFFFFFF, 3), (len(keys[0]) - 1, 1)):
            idx2 = idx.copy(); idx2[33] = bad
            want = np.zeros(65, np.uint8); want[33] = status
            _check_rejected(eng, ks, scheme, b, idx2, want, f"index {bad}")


def test_stale_handle_returns_minus_one(eng):
    from jubjub_schnorr_amd import _ffi
    b = make_batch("single", 8, seed=44, n_keys=2, mix=False)
    keys, idx = register_cols("single", b)
    ks = eng.keyset("single", *keys)
    handle = ks.handle
    ks.close()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    verdict = ctypes.c_int(-7)
    rc = _ffi.lib().jjs_keyset_verify_all(handle, 0, p(idx), p(b["u"]), p(b["R"]), None, p(b["m"]), 8, None, ctypes.byref(verdict))
    assert rc == -1
    d = [dev(x) for x in (idx, b["u"], b["R"], b["m"])]
    out = dev(np.zeros(1, np.int32))
    rc = _ffi.lib().jjs_keyset_verify_all_dev(handle, 0, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, d[3].data_ptr(), 8,
                                              out.data_ptr(), None)
    assert rc == -1


def test_four_threads_at_once(eng):
    work = []
    for t in range(4):
        scheme = SCHEMES[t % 3]
        good = make_batch(scheme, 300, seed=60 + t, n_keys=50, mix=False)
        bad = spoil_cases(scheme, good)[t][1]
        keys, idx = register_cols(scheme, good)
        work.append((scheme, eng.keyset(scheme, *keys), idx, good, bad))
    errors = []

    def worker(k):
        try:
            scheme, ks, idx, good, bad = work[k]
            for _ in range(3):
                for b, want in ((good, True), (bad, False)):
                    ok, _ = ks.verify_all(idx, *sig_cols(eng, scheme, b, "affine"), statuses_on_failure=False)
                    assert ok == want, (k, scheme, want)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for w in work:
        w[1].close()
    assert not errors, errors


def test_verdict_algorithm_forced():
    p = subprocess.run([sys.executable, os.path.join(HERE, "keyset_verify_all_child.py")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]

"""Registered key sets on the MI355X (jjs_keyset_*): statuses and tallies against the oracle and against the inline entry
point of the same format fed the same items, both variants (latency up to 16 384 items, large beyond), resident and host
calls, lifetime (destroy while a call is queued, shutdown) and threads."""
import ctypes
import threading

import numpy as np
import pytest

import jjs_oracle as o
from helpers import ARG_ORDER, make_batch, oracle_verify, to_extended, to_wire

pytestmark = pytest.mark.gpu
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def register_cols(scheme, b):
    """The distinct keys of a batch (the key columns side by side) and each item's index among them."""
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in KEYCOLS[scheme]], 1))
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    return [np.ascontiguousarray(uniq[:, 64 * i:64 * i + 64]) for i in range(len(KEYCOLS[scheme]))], inv.reshape(-1).astype(np.uint32)


def sig_cols(scheme, b, fmt, rng):
    if fmt == "affine":
        return [b["u"]] + [b[k] for k in RCOLS[scheme]] + [b["m"]]
    if fmt == "ext":
        return [b["u"]] + [to_extended(b[k], rng) for k in RCOLS[scheme]] + [b["m"]]
    sig, _, m = to_wire(scheme, b)
    return [sig, m]


def inline(eng, scheme, fmt, b, keys_fmt_cols, idx, sigs):
    """The existing entry point of the signature's format, each item given its registered key inline."""
    if fmt == "wire":
        return eng.verify_wire(scheme, sigs[0], keys_fmt_cols[0][idx], sigs[1])
    args = dict(zip(["u"] + RCOLS[scheme], sigs[:-1]), m=sigs[-1])
    for k, col in zip(KEYCOLS[scheme], keys_fmt_cols):
        args[k] = col[idx]
    arrays = [args[k] for k in ARG_ORDER[scheme]]
    return eng.verify_ext(scheme, *arrays) if fmt == "ext" else eng.verify(scheme, *arrays)


def keys_in_format(scheme, cols, fmt, rng):
    if fmt == "affine":
        return cols
    if fmt == "ext":
        return [to_extended(c, rng) for c in cols]
    comp = to_wire(scheme, {**{k: c for k, c in zip(KEYCOLS[scheme], cols)}, "u": np.zeros((len(cols[0]), 32), np.uint8),
                            "R": cols[0], "Rp": cols[0], "m": np.zeros((len(cols[0]), 32), np.uint8)})[1]
    return [np.ascontiguousarray(comp)]


def tally_of(st):
    return np.bincount(st, minlength=4)[:4]


@pytest.mark.parametrize("fmt", ["affine", "ext", "wire"])
@pytest.mark.parametrize("scheme", ["single", "double", "vargen"])
@pytest.mark.parametrize("n", [1, 64, 16384, 16385])
def test_keyset_matches_inline_and_oracle(eng, scheme, fmt, n):
    rng = np.random.default_rng(n)
    b = make_batch(scheme, n, seed=100 + n, n_keys=16)
    cols, idx = register_cols(scheme, b)
    kcols = keys_in_format(scheme, cols, fmt, rng)
    sigs = sig_cols(scheme, b, fmt, rng)
    want, _ = inline(eng, scheme, fmt, b, kcols, idx, sigs)
    if fmt == "affine":
        np.testing.assert_array_equal(want, oracle_verify(scheme, b))
    with eng.keyset(scheme, kcols[0], kcols[1] if len(kcols) > 1 else None, fmt=fmt) as ks:
        st, tally = ks.verify(dev(idx), *[dev(c) for c in sigs], fmt=fmt)
        np.testing.assert_array_equal(st.cpu().numpy(), want)
        np.testing.assert_array_equal(tally.cpu().numpy(), tally_of(want))
        if n in (64, 16385):
            hst, htally = ks.verify(idx, *sigs, fmt=fmt)
            np.testing.assert_array_equal(hst, want)
            np.testing.assert_array_equal(htally, tally_of(want))
        info = ks.info()
        small = n <= 16384
        assert info["small_calls" if small else "large_calls"] >= 1 and info["large_calls" if small else "small_calls"] == 0
        assert info["window_bits"] == 6 and info["keys"] == len(cols[0])


@pytest.mark.parametrize("scheme,n,n_keys", [("single", 1 << 17, 1 << 15), ("double", 33792, 1 << 11), ("vargen", 33792, 1 << 11)])
def test_large_call_and_out_of_range_indices(eng, scheme, n, n_keys):
    """The large variant; single signatures: 2^17 items over 2^15 keys, which repeat 4 times per call (the inline call takes
    the per-lane path).  The other schemes with fewer items: the suite's time budget."""
    b = make_batch(scheme, n, seed=9, n_keys=n_keys)
    cols, idx = register_cols(scheme, b)
    want = oracle_verify(scheme, b)
    bad = np.arange(0, n, 997)
    idx2 = idx.copy()
    idx2[bad] = len(cols[0]) + np.arange(len(bad), dtype=np.uint32)          # beyond the set
    idx2[bad[::2]] = 0xFFFFFFFF
    want2 = want.copy(); want2[bad] = 3
    sigs = sig_cols(scheme, b, "affine", None)
    with eng.keyset(scheme, *cols) as ks:
        for i in (idx, idx2):
            st, tally = ks.verify(dev(i), *[dev(c) for c in sigs])
            w = want if i is idx else want2
            np.testing.assert_array_equal(st.cpu().numpy(), w)
            np.testing.assert_array_equal(tally.cpu().numpy(), tally_of(w))
        assert ks.info()["large_calls"] == 2
        # the latency variant with indices out of range
        st, _ = ks.verify(dev(idx2[:4096]), *[dev(c[:4096]) for c in sigs])
        np.testing.assert_array_equal(st.cpu().numpy(), want2[:4096])
        assert ks.info()["small_calls"] == 1


def test_key_status_and_wire_keys_with_affine_signatures(eng):
    for scheme in ("single", "double", "vargen"):
        b = make_batch(scheme, 512, seed=31, n_keys=8)
        cols, idx = register_cols(scheme, b)
        wire_keys = keys_in_format(scheme, cols, "wire", None)[0]
        sigs = sig_cols(scheme, b, "affine", None)
        want = oracle_verify(scheme, b)
        with eng.keyset(scheme, wire_keys, fmt="wire") as ks, eng.keyset(scheme, *cols) as ka:
            # a key's own status: the oracle's verdict on the points (valid, not `is_valid`, malformed)
            for k in range(len(cols[0])):
                pts = [o.point_is_valid(tuple(int.from_bytes(c[k][h:h + 32].tobytes(), "little") for h in (0, 32))) for c in cols]
                assert ka.key_status[k] == (0 if all(pts) else 1), (scheme, k)
            st_a, _ = ka.verify(idx, *sigs)
            np.testing.assert_array_equal(st_a, want)
            # decoded wire keys: an undecodable encoding is malformed, otherwise the statuses of the affine set
            st_w, _ = ks.verify(idx, *sigs)
            undecodable = ks.key_status == 3
            np.testing.assert_array_equal(st_w[~undecodable[idx]], want[~undecodable[idx]])
            assert (st_w[undecodable[idx]] == 3).all()


def test_two_streams_one_keyset(eng):
    import torch
    b1 = make_batch("single", 20000, seed=41, n_keys=64)
    b2 = make_batch("single", 3000, seed=41, n_keys=64, mix=False)       # same keys, other signatures
    cols, idx1 = register_cols("single", b1)
    order = {r.tobytes(): i for i, r in enumerate(cols[0])}
    idx2 = np.array([order[r.tobytes()] for r in b2["PK"]], np.uint32)
    with eng.keyset("single", cols[0]) as ks:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ins1 = [dev(x) for x in (idx1, b1["u"], b1["R"], b1["m"])]
        ins2 = [dev(x) for x in (idx2, b2["u"], b2["R"], b2["m"])]
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            r1 = ks.verify(*ins1)
        with torch.cuda.stream(s2):
            r2 = ks.verify(*ins2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(r1[0].cpu().numpy(), oracle_verify("single", b1))
        np.testing.assert_array_equal(r2[0].cpu().numpy(), oracle_verify("single", b2))


def test_destroy_while_a_call_is_queued(eng):
    import torch
    b = make_batch("double", 1 << 15, seed=51, n_keys=256)
    cols, idx = register_cols("double", b)
    ins = [dev(x) for x in [idx] + sig_cols("double", b, "affine", None)]
    ks = eng.keyset("double", *cols)
    handle = ks.handle
    torch.cuda.synchronize()
    st, tally = ks.verify(*ins)
    ks.close()                                   # the launches above still read the tables
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st.cpu().numpy(), oracle_verify("double", b))
    lib = eng._lib
    out = (ctypes.c_uint64 * 7)()
    assert lib.jjs_keyset_info(handle, out) == -1
    assert lib.jjs_keyset_destroy(handle) == -1
    assert lib.jjs_keyset_destroy(0) == -1
    assert lib.jjs_keyset_verify(handle, 0, None, None, None, None, None, 0, None, None) == -1
    eng.trim()


def test_threads_share_a_keyset_while_another_is_created_and_destroyed(eng):
    b = make_batch("vargen", 4096, seed=61, n_keys=32)
    cols, idx = register_cols("vargen", b)
    sigs = sig_cols("vargen", b, "affine", None)
    want = oracle_verify("vargen", b)
    errors = []
    with eng.keyset("vargen", *cols) as ks:
        def caller(t):
            try:
                for r in range(3):
                    lo = (t * 512 + r * 128) % 4096
                    sl = slice(lo, lo + 1024)
                    st, _ = ks.verify(idx[sl], *[c[sl] for c in sigs])
                    if not np.array_equal(st, want[sl]):
                        errors.append((t, r))
            except Exception as e:          # noqa: BLE001
                errors.append(repr(e))

        def churn():
            try:
                for _ in range(4):
                    with eng.keyset("single", b["PK"][:64]) as other:
                        other.info()
            except Exception as e:          # noqa: BLE001
                errors.append(repr(e))

        threads = [threading.Thread(target=caller, args=(t,)) for t in range(8)] + [threading.Thread(target=churn)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert errors == []


def test_zero_handle_and_stale_handle_after_shutdown(eng):
    """Last in this module: the engine is shut down and brought up again."""
    lib = eng._lib
    out = (ctypes.c_uint64 * 7)()
    assert lib.jjs_keyset_info(0, out) == -1
    b = make_batch("single", 64, seed=71, n_keys=4)
    ks = eng.keyset("single", b["PK"])
    handle = ks.handle
    lib.jjs_shutdown()
    assert lib.jjs_keyset_info(handle, out) == -4
    assert lib.jjs_keyset_verify(handle, 0, None, None, None, None, None, 0, None, None) == -4
    assert lib.jjs_init(1) == 0
    assert lib.jjs_keyset_info(handle, out) == -1
    assert lib.jjs_keyset_destroy(handle) == -1
    ks.handle = 0

"""Key sets by key on the MI355X (jjs_keyset_find*, jjs_keyset_verify_keys*): the lookup against the dict of
keyset_lookup_cases.py for every scheme, registration format and query format; the resident by-key call against the
by-index call fed the dict's indices; the host call byte for byte against the inline host call; lifetime; then
keyset_lookup_child.py checks the crafted tables of the CPU cases with the hash seed pinned."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import jjs_oracle as o
import keyset_lookup_cases as kc
from helpers import ARG_ORDER, IDENT, fe_bytes, make_batch, to_extended, to_wire

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}
SCHEMES = ["single", "double", "vargen"]
FMTS = ["affine", "ext", "wire"]
MISS = kc.MISS
_honest = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def idx_of(t):
    """The int32 tensor of a resident call as the uint32 indices it holds."""
    return t.cpu().numpy().view(np.uint32)


def honest_keys(scheme):
    """1 100 distinct valid keys of the scheme, as rows of its key columns side by side."""
    if scheme not in _honest:
        b = make_batch(scheme, 1100, seed=77, n_keys=1100, mix=False)
        rows = [r.tobytes() for r in np.concatenate([b[k] for k in KEYCOLS[scheme]], 1)]
        assert len(set(rows)) == len(rows)
        _honest[scheme] = rows
    return _honest[scheme]


def tally_of(st):
    return np.bincount(st, minlength=7)[:4]


@pytest.mark.parametrize("reg", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_find_against_the_dict(eng, scheme, reg):
    """Sets of 1, 3, 5, 64 and 1 000 keys with duplicates, invalid, off-curve and malformed members, registered in `reg`;
    queries in every format; 0, 1, 63, 64, 65 and 257 of them; resident and host calls."""
    import torch
    honest = honest_keys(scheme)
    cols = len(KEYCOLS[scheme])
    for nk in (1, 3, 5, 64, 1000):
        rng = np.random.default_rng(nk)
        create, held, bad = kc.registered_set(honest, nk, reg, rng)
        with eng.keyset(scheme, create[0], create[1], fmt=reg) as ks:
            assert ((ks.key_status == 3) == (np.array(bad) == 1)).all(), (nk, "the keys the model holds as malformed")
            for qf in FMTS:
                pool = kc.query_pool(honest, held, qf, rng)
                want = kc.want(held, qf, pool, bad)
                assert 0 < (want != MISS).sum() < len(want)
                for n in (0, 1, 63, 64, 65, 257):
                    q = kc.query_columns(pool[:n], cols, qf)
                    got = ks.find(*[dev(c) for c in q], fmt=qf)
                    torch.cuda.synchronize()
                    np.testing.assert_array_equal(idx_of(got), want[:n], err_msg=f"dev nk={nk} {qf} n={n}")
                    if n in (0, 65, 257):
                        np.testing.assert_array_equal(ks.find(*q, fmt=qf), want[:n], err_msg=f"host nk={nk} {qf} n={n}")
            info = ks.info()
            assert info["small_calls"] == info["large_calls"] == 0, "a lookup is no verification call"


def by_key_batch(scheme, n, n_keys, registered, seed):
    """n items over n_keys honest keys of which the first `registered` are in the set, beside a registered identity and a
    registered key with u = q (malformed: never found); some items name those two.  Returns (batch, the set's affine
    columns, the rows the set holds, their malformed flags)."""
    b = make_batch(scheme, n, seed=seed, n_keys=n_keys)
    names = KEYCOLS[scheme]
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in names], 1))
    kk = min(n_keys, n)                    # make_batch draws its keys first: the same seed and key count give the same keys
    honest = np.ascontiguousarray(np.concatenate([make_batch(scheme, kk, seed=seed, n_keys=kk, mix=False)[k] for k in names], 1))
    reg = honest[:min(registered, kk)]
    ident = reg[:1].copy(); ident[0, :64] = IDENT
    nc = reg[:1].copy(); nc[0, :32] = fe_bytes(o.Q)
    reg = np.concatenate([reg, ident, nc])
    if n >= 40:
        cat[np.arange(5, n, 19)] = reg[-2]
        cat[np.arange(3, n, 17)] = reg[-1]
    for i, name in enumerate(names):
        b[name] = np.ascontiguousarray(cat[:, 64 * i:64 * i + 64])
    keys = [np.ascontiguousarray(reg[:, 64 * i:64 * i + 64]) for i in range(len(names))]
    return b, keys, [r.tobytes() for r in reg], [0] * (len(reg) - 1) + [1]


def ext_rows(points, rng):
    """to_extended, but a point with a coordinate >= q keeps its bytes (Z = 1): nothing to rescale."""
    out = to_extended(points, rng)
    for i, row in enumerate(points):
        if not kc._canonical(row.tobytes()):
            out[i, :64] = row
            out[i, 64:] = 0
            out[i, 64] = 1
    return out


def call_columns(scheme, b, fmt, rng):
    """(key columns, signature columns + messages) of the by-key call in `fmt`."""
    if fmt == "affine":
        return [b[k] for k in KEYCOLS[scheme]], [b["u"]] + [b[k] for k in RCOLS[scheme]] + [b["m"]]
    if fmt == "ext":
        return [ext_rows(b[k], rng) for k in KEYCOLS[scheme]], [b["u"]] + [to_extended(b[k], rng) for k in RCOLS[scheme]] + [b["m"]]
    sig, pk, m = to_wire(scheme, b)
    return [np.ascontiguousarray(pk)], [np.ascontiguousarray(sig), m]


def expected_indices(held, bad, fmt, K):
    rows = [r.tobytes() for r in np.ascontiguousarray(np.concatenate(K, 1))]
    return kc.want(held, fmt, rows, bad)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n", [1, 65, 257, 4097, 8193, 16385])
def test_verify_keys_dev_against_the_by_index_call(eng, scheme, n):
    """Hits: exactly the status of jjs_keyset_verify_dev with the dict's index; misses: 6, in no tally word.  The latency
    variant at its three position counts (16 up to 2 048 items, 8 up to 8 192, 4 beyond) and the smallest large call."""
    import torch
    b, keys, held, bad = by_key_batch(scheme, n, 48, 32, seed=200 + n)
    rng = np.random.default_rng(n)
    for fmt in (FMTS if n in (257, 16385) else ["affine"]):
        K, sigs = call_columns(scheme, b, fmt, rng)
        found = expected_indices(held, bad, fmt, K)
        miss = found == MISS
        assert n < 40 or (miss.any() and (~miss).any())
        with eng.keyset(scheme, *keys) as ks:
            ref, _ = ks.verify(dev(found.view(np.int32)), *[dev(c) for c in sigs], fmt=fmt)      # (a miss: beyond the set, 3)
            want = np.where(miss, 6, ref.cpu().numpy()).astype(np.uint8)
            assert (ref.cpu().numpy()[miss] == 3).all()
            before = ks.info()
            st, tally, idx = ks.verify_keys([dev(c) for c in K], *[dev(c) for c in sigs], fmt=fmt, want_idx=True)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(idx_of(idx), found, err_msg=f"{fmt}")
            np.testing.assert_array_equal(st.cpu().numpy(), want, err_msg=f"{fmt}")
            np.testing.assert_array_equal(tally.cpu().numpy(), tally_of(want))
            assert int(tally.sum()) == n - int(miss.sum())
            # idx_out NULL, and no status column: the tally alone
            st2, tally2 = ks.verify_keys([dev(c) for c in K], *[dev(c) for c in sigs], fmt=fmt)
            _, tally3 = ks.verify_keys([dev(c) for c in K], *[dev(c) for c in sigs], fmt=fmt, want_status=False)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(st2.cpu().numpy(), want)
            np.testing.assert_array_equal(tally2.cpu().numpy(), tally_of(want))
            np.testing.assert_array_equal(tally3.cpu().numpy(), tally_of(want))
            after = ks.info()
            which = "small_calls" if n <= 16384 else "large_calls"
            assert after[which] - before[which] == 3 and after["small_calls"] + after["large_calls"] - before["small_calls"] - before["large_calls"] == 3


def inline_host(eng, scheme, fmt, K, sigs):
    if fmt == "wire":
        return eng.verify_wire(scheme, sigs[0], K[0], sigs[1])
    args = dict(zip(["u"] + RCOLS[scheme], sigs[:-1]), m=sigs[-1])
    args.update(zip(KEYCOLS[scheme], K))
    arrays = [args[k] for k in ARG_ORDER[scheme]]
    return eng.verify_ext(scheme, *arrays) if fmt == "ext" else eng.verify(scheme, *arrays)


def moving_stats(eng):
    s = eng.path_stats()           # what an inline host call moves: the lanes' counters and the paths'
    return {k: s[k] for k in ("latency", "throughput", "lane_launches", "lane_calls")}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_verify_keys_is_the_inline_host_call(eng, scheme, fmt):
    """300 items mixing registered, unregistered, invalid and malformed keys and bad signatures: statuses and tally byte for
    byte those of the inline host call.  The same batch with every key registered: no inline call runs."""
    rng = np.random.default_rng(300)
    b, keys, held, bad = by_key_batch(scheme, 300, 48, 32, seed=301)
    K, sigs = call_columns(scheme, b, fmt, rng)
    want, want_tally = inline_host(eng, scheme, fmt, K, sigs)
    assert len(set(want.tolist())) >= 3
    found = expected_indices(held, bad, fmt, K)
    assert (found == MISS).sum() >= 50 and (found != MISS).sum() >= 100
    with eng.keyset(scheme, *keys) as ks:
        before = moving_stats(eng)
        st, tally, idx = ks.verify_keys(K, *sigs, fmt=fmt, want_idx=True)
        np.testing.assert_array_equal(idx, found)
        np.testing.assert_array_equal(st, want)
        np.testing.assert_array_equal(tally, want_tally)
        assert moving_stats(eng) != before, "the missed rows went through an inline host call"
    # every key registered (the set holds what the items carry, the malformed key included: its items miss and would go
    # inline, so the batch here is the one without it)
    keep = np.all([[kc._canonical(r.tobytes()) for r in b[k]] for k in KEYCOLS[scheme]], axis=0)
    b2 = {k: np.ascontiguousarray(v[keep]) for k, v in b.items()}
    K2, sigs2 = call_columns(scheme, b2, fmt, rng)
    want2, want_tally2 = inline_host(eng, scheme, fmt, K2, sigs2)
    cat = np.ascontiguousarray(np.concatenate([b2[k] for k in KEYCOLS[scheme]], 1))
    uniq = np.unique(cat, axis=0)
    with eng.keyset(scheme, *[np.ascontiguousarray(uniq[:, 64 * i:64 * i + 64]) for i in range(len(KEYCOLS[scheme]))]) as ks:
        before = moving_stats(eng)
        st, tally, idx = ks.verify_keys(K2, *sigs2, fmt=fmt, want_idx=True)
        assert moving_stats(eng) == before, "no inline call when every key is registered"
        assert (idx != MISS).all()
        np.testing.assert_array_equal(st, want2)
        np.testing.assert_array_equal(tally, want_tally2)
        st, tally = ks.verify_keys(K2, *sigs2, fmt=fmt, want_status=True)
        np.testing.assert_array_equal(st, want2)


def test_a_destroyed_set_and_two_sets_alive(eng):
    import torch
    from jubjub_schnorr_amd import _ffi
    honest = honest_keys("single")
    rows = np.frombuffer(b"".join(honest[:200]), np.uint8).reshape(200, 64)
    a, b = eng.keyset("single", rows[:100]), eng.keyset("single", rows[100:])
    q = np.ascontiguousarray(rows[90:110])
    np.testing.assert_array_equal(a.find(q), [90 + i if i < 10 else MISS for i in range(20)])
    np.testing.assert_array_equal(b.find(q), [MISS if i < 10 else i - 10 for i in range(20)])
    np.testing.assert_array_equal(idx_of(a.find(dev(q))), a.find(q))
    handle = a.handle
    a.close()
    lib = _ffi.lib()
    out = np.zeros(20, np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    d = dev(q); dout = torch.zeros(20, dtype=torch.int32, device="cuda")
    assert lib.jjs_keyset_find(handle, 0, p(q), None, 20, p(out)) == -1
    assert lib.jjs_keyset_find_dev(handle, 0, d.data_ptr(), None, 20, dout.data_ptr(), None) == -1
    assert lib.jjs_keyset_verify_keys(handle, 0, p(q), None, p(q), p(q), None, p(q), 20, p(out), None, None) == -1
    assert lib.jjs_keyset_verify_keys_dev(handle, 0, d.data_ptr(), None, d.data_ptr(), d.data_ptr(), None, d.data_ptr(), 20, None, None, None, None) == -1
    np.testing.assert_array_equal(b.find(q), [MISS if i < 10 else i - 10 for i in range(20)])
    # n == 0 and a NULL column the format needs: as jjs_keyset_verify(_dev)
    assert lib.jjs_keyset_find(b.handle, 0, None, None, 0, None) == 0 and lib.jjs_keyset_find(b.handle, 3, None, None, 0, None) == -1
    assert lib.jjs_keyset_find(b.handle, 0, None, None, 20, p(out)) == -1
    assert lib.jjs_keyset_verify_keys(b.handle, 0, p(q), None, p(q), None, None, p(q), 20, p(out), None, None) == -1
    t = np.ones(4, np.uint64)
    assert lib.jjs_keyset_verify_keys(b.handle, 0, None, None, None, None, None, None, 0, None, p(t), None) == 0 and not t.any()
    b.close()


def test_crafted_tables_with_the_seed_pinned():
    p = subprocess.run([sys.executable, os.path.join(HERE, "keyset_lookup_child.py")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]

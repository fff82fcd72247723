"""Adding keys to a live key set on the MI355X (jjs_keyset_add, jjs_keyset_reserve, jjs_keyset_growth): a set that grew by
JJS_KEYSET_ADD_APPEND against jjs_keyset_create of the same keys, byte for byte through every call that takes a set, in place
and moving; JJS_KEYSET_ADD_UNIQUE against the Python dict of keyset_add_cases.py; stale handles and no-ops; then
keyset_add_child.py verifies against old indices from four threads while a fifth adds."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import keyset_add_cases as ac
import keyset_lookup_cases as kc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMES = ["single", "double", "vargen"]
FMTS = ["affine", "ext", "wire"]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def key_columns(rows, scheme, fmt, z0=3):
    return ac.columns([ac.encode_key(r, fmt, z0 + 2 * i) for i, r in enumerate(rows)], scheme, fmt)


def same_set(a, b, scheme, rows, calls, label):
    """Every call that takes a set gives the same bytes on `a` and `b`.  rows: the affine rows both hold (queries);
    calls: [(key_idx, signature columns, oracle statuses or None)]."""
    ia, ib = a.info(), b.info()
    assert (ia["keys"], ia["valid_keys"], ia["scheme"]) == (ib["keys"], ib["valid_keys"], ib["scheme"]), label
    np.testing.assert_array_equal(a.key_status, b.key_status, err_msg=label)
    canon = [r if all(kc._canonical(p) for p in ac._pts(r)) else kc.IDENT * ac.COLS[scheme] for r in rows]       # (an ext / wire query needs a point)
    stranger = ac.key_rows(ac.COLS[scheme], 7000, 1)
    for qf in FMTS:
        q = [c for c in key_columns((rows if qf == "affine" else canon) + stranger, scheme, qf, z0=5) if c is not None]
        fa, fb = a.find(*q, fmt=qf), b.find(*q, fmt=qf)
        np.testing.assert_array_equal(fa, fb, err_msg=f"{label} find {qf}")
        assert fa[-1] == kc.MISS and (fa[:-1] != kc.MISS).sum() >= len(rows) - 3       # (a malformed key, Z = 0, an off-curve point may miss)
    for idx, sig, want in calls:
        sa, ta = a.verify(idx, *sig)
        sb, tb = b.verify(idx, *sig)
        np.testing.assert_array_equal(sa, sb, err_msg=f"{label} verify n={len(idx)}")
        np.testing.assert_array_equal(ta, tb)
        if want is not None:
            np.testing.assert_array_equal(sa, want, err_msg=f"{label} verify n={len(idx)} against the oracle")
    idx, sig, _ = calls[0]
    named = np.frombuffer(b"".join(rows[min(int(i), len(rows) - 1)] for i in idx), np.uint8).reshape(len(idx), -1)
    K = [np.ascontiguousarray(named[:, 64 * c:64 * c + 64]) for c in range(ac.COLS[scheme])]
    ka, kb = a.verify_keys(K, *sig, want_idx=True), b.verify_keys(K, *sig, want_idx=True)
    for x, y in zip(ka, kb):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} verify_keys")
    good = a.verify(idx, *sig)[0] == 0
    for pick in (np.ones(len(idx), bool), good):
        va = a.verify_all(idx[pick], *[c[pick] for c in sig])
        vb = b.verify_all(idx[pick], *[c[pick] for c in sig])
        assert va[0] == vb[0] and (va[1] is None) == (vb[1] is None) and (va[1] is None or (va[1] == vb[1]).all()), f"{label} verify_all"
    assert va[0] is True or not good.any(), "the items the set accepts one by one are accepted as a batch"
    if scheme != "single":
        return
    # the multisignature calls over committees drawn from the set: shares that do not verify still read every key, flag and table
    rng = np.random.default_rng(len(rows))
    sizes = rng.integers(1, 5, 24)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    N, B = int(offs[-1]), len(sizes)
    kidx = rng.integers(0, len(rows), N).astype(np.uint32)
    kidx[offs[3]] = len(rows)                      # one committee names an index beyond the set
    z = ac.signed_batch("single", 16385, 8, 900)[0]["u"][:N]
    R = ac.signed_batch("single", 16385, 8, 900)[0]["R"][:N]
    S = ac.signed_batch("single", 16385, 8, 900)[0]["R"][N:2 * N]
    m = ac.signed_batch("single", 16385, 8, 900)[0]["m"][:B]
    for x, y in zip(a.multisig_combine(kidx, z, R, S, m, offs), b.multisig_combine(kidx, z, R, S, m, offs)):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} multisig_combine")
    pa, pb = a.multisig_aggregate_pk(kidx, offs), b.multisig_aggregate_pk(kidx, offs)
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} multisig_aggregate_pk")
    for x, y in zip(a.multisig_verify(kidx, offs, z[:B], R[:B], m), b.multisig_verify(kidx, offs, z[:B], R[:B], m)):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} multisig_verify")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_append_equals_create(eng, scheme, fmt):
    """A = create(K1), add(K2), add(K3); B = create(K1 ++ K2 ++ K3); |K1| in {1, 3, 4}, |K2| = 1 (a malformed key), |K3| = 5 (a
    status-1 key and a duplicate among them): the 8-to-16-slot step of the lookup table at 4 -> 5 keys, moving adds and -- behind
    reserve(16) -- adds in place, the path asserted through jjs_keyset_growth."""
    for k1 in (1, 3, 4):
        rows, where, s1, mal = ac.append_keys(scheme, k1)
        calls = [ac.items_over(scheme, rows, where, s1, mal, 64), ac.items_over(scheme, rows, where, s1, mal, 16385, oracle=k1 == 4)]
        c0, c1 = key_columns(rows, scheme, fmt)
        cut = lambda c, lo, hi: None if c is None else np.ascontiguousarray(c[lo:hi])  # noqa: E731
        with eng.keyset(scheme, c0, c1, fmt=fmt) as b:
            assert b.key_status[mal] == 3 and b.key_status[s1] == 1 and (np.delete(b.key_status, [mal, s1]) == 0).all()
            assert b.growth() == {"capacity": k1 + 6, "add_calls": 0, "relocations": 0, "lookup_rebuilds": 0, "add_known": 0}
            for reserve in (False, True):
                label = f"{scheme} {fmt} k1={k1} reserve={reserve}"
                with eng.keyset(scheme, cut(c0, 0, k1), cut(c1, 0, k1), fmt=fmt) as a:
                    created_bytes = a.info()["device_bytes"]
                    if reserve:
                        a.reserve(16)
                        assert a.growth()["capacity"] == 16 and a.growth()["relocations"] == 1
                        a.reserve(9)
                        assert a.growth()["capacity"] == 16 and a.growth()["relocations"] == 1, "a set that has that much: nothing happens"
                    else:
                        assert a.info()["device_bytes"] == created_bytes and a.growth()["capacity"] == k1
                    idx, st = a.add(cut(c0, k1, k1 + 1), cut(c1, k1, k1 + 1), fmt=fmt)
                    assert idx.tolist() == [k1] and st.tolist() == [3], label
                    idx, st = a.add(cut(c0, k1 + 1, k1 + 6), cut(c1, k1 + 1, k1 + 6), fmt=fmt)
                    assert idx.tolist() == list(range(k1 + 1, k1 + 6)) and st.tolist() == b.key_status[k1 + 1:].tolist(), label
                    g = a.growth()
                    rebuilds = sum(kc.slot_count(x) != kc.slot_count(y) for x, y in ((k1, k1 + 1), (k1 + 1, k1 + 6)))
                    cap = 16 if reserve else max(k1 + 6, max(k1 + 1, k1 + k1 // 2) + max(k1 + 1, k1 + k1 // 2) // 2)
                    assert g == {"capacity": cap, "add_calls": 2, "relocations": 1 if reserve else 2, "lookup_rebuilds": rebuilds, "add_known": 0}, (label, g)
                    same_set(a, b, scheme, rows, calls, label)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_unique_against_the_dict(eng, scheme, fmt):
    """The candidate lists of the host test at 257 and 65 537 candidates: idx_out, key_status, n_added, JJS_KEYSET_ADD_KNOWN and
    the set afterwards against the model and against jjs_keyset_create of the model's key list."""
    held, bad = ac.base_set(scheme)
    cols = ac.COLS[scheme]
    calls = [ac.items_over(scheme, held, {}, 0, 3, 64, oracle=False)]
    for n in (257, 65537, 0):         # 0: the spread list -- first occurrences in every wave of several blocks, 300 new keys
        encs = ac.candidates(scheme, fmt, n) if n else ac.spread_candidates(scheme, fmt)
        rows = [ac.canonical_row(e, fmt) for e in encs]
        want_idx, new, known = ac.unique_model(held, bad, rows)
        assert known > 0 and len(new) >= 6 and (want_idx == ac.MISS).any() and (want_idx == 1).any()
        assert n or len(new) > 256 + 6
        with eng.keyset(scheme, *ac.row_columns(held, cols)) as a:
            idx, st = a.add(*ac.columns(encs, scheme, fmt), fmt=fmt, unique=True)
            np.testing.assert_array_equal(idx, want_idx, err_msg=f"n={n}")
            assert st.tolist() == [3 if r is None else ac.row_status(r) for r in rows]
            g = a.growth()
            assert a.n_keys == len(held) + len(new) == a.info()["keys"] and g["add_known"] == known and g["add_calls"] == 1
            with eng.keyset(scheme, *ac.row_columns(held + new, cols)) as b:
                same_set(a, b, scheme, held + new, calls, f"{scheme} {fmt} unique n={n}")
            # the same candidates again: every one of them is known now, and nothing moves
            idx2, st2 = a.add(*ac.columns(encs, scheme, fmt), fmt=fmt, unique=True)
            np.testing.assert_array_equal(idx2, want_idx)
            assert st2.tolist() == st.tolist() and a.n_keys == len(held) + len(new)
            g2 = a.growth()
            assert g2["add_known"] == known + int((want_idx != ac.MISS).sum()) and g2["relocations"] == g["relocations"]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_append_of_more_than_a_block_equals_create(eng, scheme, fmt):
    """The spread list appended in one call, 1 300 keys with malformed, invalid and repeated ones among them -- the chain, flag
    and table kernels over a shifted range of several blocks, the lookup table rebuilt -- then 300 more in place behind a
    reserve (the ranged insert at an offset, several blocks of it): against jjs_keyset_create of the same keys."""
    held, bad = ac.base_set(scheme)
    cols = ac.COLS[scheme]
    encs = ac.spread_candidates(scheme, fmt)
    more = [ac.encode(r, fmt, 77 + i) for i, r in enumerate(ac.key_rows(cols, 9000, 3) + ac.chain_rows(cols, ac.SPREAD_KEYS)[:297])]
    head = [ac.encode_key(r, fmt, 3 + i) for i, r in enumerate(held)]
    calls = [ac.items_over(scheme, held, {}, 0, 3, 64, oracle=False)]
    with eng.keyset(scheme, *ac.columns(head, scheme, fmt), fmt=fmt) as a, eng.keyset(scheme, *ac.columns(head + encs + more, scheme, fmt), fmt=fmt) as b:
        idx, st = a.add(*ac.columns(encs, scheme, fmt), fmt=fmt)
        assert idx.tolist() == list(range(len(held), len(held) + len(encs))) and st.tolist() == b.key_status[len(held):len(held) + len(encs)].tolist()
        assert set(st.tolist()) == {0, 1, 3}
        n1 = len(held) + len(encs)
        a.reserve(n1 + 1000)
        idx, st = a.add(*ac.columns(more, scheme, fmt), fmt=fmt)
        assert idx.tolist() == list(range(n1, n1 + 300)) and not st.any()
        g = a.growth()
        assert g == {"capacity": n1 + 1000, "add_calls": 2, "relocations": 2, "lookup_rebuilds": 1, "add_known": 0}, g
        rows = [ac.canonical_row(e, fmt) for e in encs + more]
        queries = list(dict.fromkeys(held + [r for r in rows if r is not None]))
        same_set(a, b, scheme, queries[:40] + queries[-40:], calls, f"{scheme} {fmt} append of blocks")
        # every registered key is found at the lowest index that holds it, on both
        want = kc.want(held + [r or held[3] for r in rows], "affine", queries, bad + [int(r is None) for r in rows])
        q = [c for c in ac.row_columns(queries, cols) if c is not None]
        np.testing.assert_array_equal(a.find(*q), want)
        np.testing.assert_array_equal(b.find(*q), want)


def test_stale_handles_and_no_ops(eng):
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _, h = ac.signed_batch("single", 16385, 8, 900)
    keys = np.frombuffer(b"".join(h), np.uint8).reshape(8, 64)
    idx, sig, want = ac.items_over("single", h, {j: j for j in range(8)}, 0, 0, 64, seed=900, oracle=False)
    idx = (np.arange(64) % 4).astype(np.uint32)
    a = eng.keyset("single", keys[:4])
    ref = a.verify(idx, *sig)[0]
    before = (a.info(), a.growth())
    added = ctypes.c_size_t(99)
    assert lib.jjs_keyset_add(a.handle, 0, None, None, 0, 0, None, None, ctypes.byref(added)) == 0 and added.value == 0
    assert lib.jjs_keyset_add(a.handle, 0, None, None, 0, 1, None, None, None) == 0
    assert (a.info(), a.growth()) == before, "n == 0 changes nothing"
    assert lib.jjs_keyset_add(a.handle, 0, p(keys), None, 1, 2, None, None, None) == -1, "an unknown mode"
    assert lib.jjs_keyset_add(a.handle, 3, p(keys), None, 1, 0, None, None, None) == -1
    assert lib.jjs_keyset_add(a.handle, 0, None, None, 1, 0, None, None, None) == -1
    assert lib.jjs_keyset_add(a.handle, 0, p(keys), None, (1 << 24) - 3, 0, None, None, None) == -1, "n_old + n beyond 2^24"
    assert lib.jjs_keyset_reserve(a.handle, (1 << 24) + 1) == -1
    assert (a.info(), a.growth()) == before
    # every output is nullable; a moving add, then jjs_trim frees the allocation it left: the set stays usable
    assert lib.jjs_keyset_add(a.handle, 0, p(np.ascontiguousarray(keys[4:])), None, 4, 0, None, None, None) == 0
    assert a.growth()["relocations"] == 1 and a.info()["keys"] == 8
    eng.trim()
    np.testing.assert_array_equal(a.verify(idx, *sig)[0], ref)
    np.testing.assert_array_equal(a.find(keys), np.arange(8))
    with eng.keyset("single", keys) as b:
        np.testing.assert_array_equal(a.verify((np.arange(64) % 8).astype(np.uint32), *sig)[0], b.verify((np.arange(64) % 8).astype(np.uint32), *sig)[0])
    handle = a.handle
    a.close()
    assert lib.jjs_keyset_add(handle, 0, p(keys), None, 1, 0, None, None, None) == -1, "add after destroy"
    assert lib.jjs_keyset_add(handle, 0, None, None, 0, 0, None, None, None) == -1
    assert lib.jjs_keyset_reserve(handle, 100) == -1 and lib.jjs_keyset_reserve(handle, 0) == -1
    assert lib.jjs_keyset_growth(handle, p(np.zeros(5, np.uint64))) == -1
    eng.trim()


def test_old_indices_under_a_concurrent_add():
    p = subprocess.run([sys.executable, os.path.join(HERE, "keyset_add_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]

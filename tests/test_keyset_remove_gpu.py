"""Removing keys from a live key set and compacting it on the MI355X (jjs_keyset_remove, jjs_keyset_compact, jjs_keyset_removal):
a set after remove(D) against jjs_keyset_create of the same keys with D's rows 0xFF, and a compacted set against
jjs_keyset_create of the survivors, byte for byte through every call that takes a set; sequences of removes, adds and a
compact against the list-and-dict model of keyset_remove_cases.py; no-ops and stale handles; then keyset_remove_child.py
verifies from five threads while a sixth removes and compacts."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import keyset_add_cases as ac
import keyset_lookup_cases as kc
import keyset_remove_cases as rc

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
    """Every call that takes a set gives the same bytes on `a` and `b`.  rows: the keys to ask for (the keys `a` was made of,
    the removed ones among them); calls: [(key_idx, signature columns, oracle statuses or None)]."""
    cols = ac.COLS[scheme]
    ia, ib = a.info(), b.info()
    assert (ia["keys"], ia["valid_keys"], ia["scheme"]) == (ib["keys"], ib["valid_keys"], ib["scheme"]), label
    np.testing.assert_array_equal(a.key_status, b.key_status, err_msg=label)
    canon = [r if all(kc._canonical(p) for p in ac._pts(r)) else kc.IDENT * cols for r in rows]       # (an ext / wire query needs a point)
    stranger = ac.key_rows(cols, 7000, 1)
    found = None
    for qf in FMTS:
        q = [c for c in key_columns((rows if qf == "affine" else canon) + stranger, scheme, qf, z0=5) if c is not None]
        fa, fb = a.find(*q, fmt=qf), b.find(*q, fmt=qf)
        np.testing.assert_array_equal(fa, fb, err_msg=f"{label} find {qf}")
        assert fa[-1] == kc.MISS
        found = fa if qf == "affine" else found
    for idx, sig, want in calls:
        sa, ta = a.verify(idx, *sig)
        sb, tb = b.verify(idx, *sig)
        np.testing.assert_array_equal(sa, sb, err_msg=f"{label} verify n={len(idx)}")
        np.testing.assert_array_equal(ta, tb)
        if want is not None:
            np.testing.assert_array_equal(sa, want, err_msg=f"{label} verify n={len(idx)} against the oracle")
    idx, sig, _ = calls[0]
    named = np.frombuffer(b"".join(rows[min(int(i), len(rows) - 1)] for i in idx), np.uint8).reshape(len(idx), -1)
    K = [np.ascontiguousarray(named[:, 64 * c:64 * c + 64]) for c in range(cols)]
    ka, kb = a.verify_keys(K, *sig, want_idx=True), b.verify_keys(K, *sig, want_idx=True)
    for x, y in zip(ka, kb):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} verify_keys")
    good = a.verify(idx, *sig)[0] == 0
    for pick in (np.ones(len(idx), bool), good):
        if not pick.any():
            continue
        va = a.verify_all(idx[pick], *[c[pick] for c in sig])
        vb = b.verify_all(idx[pick], *[c[pick] for c in sig])
        assert va[0] == vb[0] and (va[1] is None) == (vb[1] is None) and (va[1] is None or (va[1] == vb[1]).all()), f"{label} verify_all"
        assert va[0] is True or pick is not good, "the items the set accepts one by one are accepted as a batch"
    if scheme != "single":
        return found
    # the multisignature calls over committees drawn from the set: shares that do not verify still read every key, flag and table
    n_keys = ia["keys"]
    rng = np.random.default_rng(n_keys)
    sizes = rng.integers(1, 5, 24)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    N, B = int(offs[-1]), len(sizes)
    kidx = rng.integers(0, n_keys, N).astype(np.uint32)
    kidx[offs[3]] = n_keys                         # one committee names an index beyond the set
    batch = ac.signed_batch("single", 16385, 8, 900)[0]
    z, R, S, m = batch["u"][:N], batch["R"][:N], batch["R"][N:2 * N], batch["m"][:B]
    for x, y in zip(a.multisig_combine(kidx, z, R, S, m, offs), b.multisig_combine(kidx, z, R, S, m, offs)):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} multisig_combine")
    for x, y in zip(a.multisig_aggregate_pk(kidx, offs), b.multisig_aggregate_pk(kidx, offs)):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} multisig_aggregate_pk")
    for x, y in zip(a.multisig_verify(kidx, offs, z[:B], R[:B], m), b.multisig_verify(kidx, offs, z[:B], R[:B], m)):
        np.testing.assert_array_equal(x, y, err_msg=f"{label} multisig_verify")
    return found


def picked(n, names):
    return [(name, idx) for name, idx in rc.patterns(n) if names is None or name in names]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_remove_equals_create_with_ff(eng, scheme, fmt):
    """A = create(K); A.remove(D) against B = create(K with D's rows 0xFF): 4 and 5 keys (the 8- and the 16-slot table) with
    every pattern, 257 and 1 300 keys with the patterns that differ there; a 64-item call each, and a 16 385-item call (the large
    variant) once per key count.  Statuses against the oracle once per scheme."""
    for n in rc.GPU_COUNTS:
        rows, status, where = rc.gpu_set(scheme, n)
        names = None if n <= 5 else ("all_but_one", "every_second", "one_wave", "across_a_block_edge", "lowest_of_three", "two_of_three",
                                     "twice_and_out_of_range")
        for name, idx in picked(n, names):
            label = f"{scheme} {fmt} n={n} {name}"
            m = rc.Model(rows, status)
            want_res, want_n, want_valid = m.remove(idx)
            ff = rc.with_ff(rows, m.removed)
            oracle = fmt == "affine" and n == 5 and name == "every_second"
            calls = [rc.items_over(scheme, ff, where, 64, oracle=oracle)]
            if name == "every_second":
                calls.append(rc.items_over(scheme, ff, where, 16385, oracle=oracle))
            with eng.keyset(scheme, *key_columns(rows, scheme, fmt), fmt=fmt) as a, eng.keyset(scheme, *key_columns(ff, scheme, fmt), fmt=fmt) as b:
                before = a.info()
                np.testing.assert_array_equal(a.key_status, status, err_msg=label)
                res, n_removed = a.remove(idx)
                np.testing.assert_array_equal(res, want_res, err_msg=label)
                assert n_removed == want_n, label
                after = a.info()
                assert after["device_bytes"] == before["device_bytes"] and after["keys"] == n and after["valid_keys"] == before["valid_keys"] - want_valid, label
                assert a.removal() == {"removed_keys": want_n, "live_keys": n - want_n, "remove_calls": 1, "compact_calls": 0}, label
                np.testing.assert_array_equal(a.removed, m.removed, err_msg=label)
                found = same_set(a, b, scheme, rows, calls, label)
                np.testing.assert_array_equal(found[:-1], m.find(rows), err_msg=f"{label}: the lowest surviving index of every key")
                # the same indices again: nothing is left to remove, nothing changes
                mid = a.info()
                res2, n2 = a.remove(idx)
                assert n2 == 0 and set(res2.tolist()) <= {rc.WAS_REMOVED, rc.NOT_IN_RANGE} and a.info() == mid, label
                assert a.removal() == {"removed_keys": want_n, "live_keys": n - want_n, "remove_calls": 2, "compact_calls": 0}, label
            if n > 5:
                eng.trim()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_compact_equals_create_of_the_survivors(eng, scheme, fmt):
    for n in rc.GPU_COUNTS:
        rows, status, _ = rc.gpu_set(scheme, n)
        for name, idx in picked(n, ("first", "all_but_one", "every_second", "across_a_block_edge", "lowest_of_three", "the_malformed_key")):
            label = f"{scheme} {fmt} n={n} {name}"
            m = rc.Model(rows, status)
            m.remove(idx)
            want_map, after = m.compact()
            h = ac.signed_batch(scheme, 16385, 8, 900)[1]
            where = {j: [i for i, r in enumerate(after.rows) if r == h[j]] for j in range(8)}
            calls = [rc.items_over(scheme, after.rows, where, 64)]
            if name == "every_second":
                calls.append(rc.items_over(scheme, after.rows, where, 16385))
            with eng.keyset(scheme, *key_columns(rows, scheme, fmt), fmt=fmt) as a, eng.keyset(scheme, *key_columns(after.rows, scheme, fmt), fmt=fmt) as b:
                a.remove(idx)
                got_map = a.compact()
                np.testing.assert_array_equal(got_map, want_map, err_msg=label)
                assert a.n_keys == len(after) and not a.removed.any(), label
                ia, ib = a.info(), b.info()
                assert ia["device_bytes"] == ib["device_bytes"] and ia["keys"] == len(after), (label, ia, ib)
                assert a.growth() == {"capacity": len(after), "add_calls": 0, "relocations": 1, "lookup_rebuilds": 0, "add_known": 0}, label
                assert a.removal() == {"removed_keys": 0, "live_keys": len(after), "remove_calls": 1, "compact_calls": 1}, label
                found = same_set(a, b, scheme, rows, calls, label)
                np.testing.assert_array_equal(found[:-1], after.find(rows), err_msg=label)
                # compacting again: nothing is removed, the identity map, nothing moves
                np.testing.assert_array_equal(a.compact(), np.arange(len(after)))
                assert a.growth()["relocations"] == 1 and a.removal()["compact_calls"] == 1
            if n > 5:
                eng.trim()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_remove_add_remove_compact_add(eng, scheme):
    """Remove, add UNIQUE of a removed key (registered anew, at a new index), remove again, compact, add: the model at every
    step, and the set in the end against jjs_keyset_create of the model's keys."""
    cols = ac.COLS[scheme]
    for n in (5, 257):
        rows, status, _ = rc.gpu_set(scheme, n)
        t = rc.triple(n)
        m = rc.Model(rows, status)
        fresh = ac.key_rows(cols, 9100, 2)
        with eng.keyset(scheme, *ac.row_columns(rows, cols)) as a:
            def step(label):
                np.testing.assert_array_equal(a.key_status, m.key_status(), err_msg=label)
                q = list(dict.fromkeys(m.rows + fresh))
                np.testing.assert_array_equal(a.find(*[c for c in ac.row_columns(q, cols) if c is not None]), m.find(q), err_msg=label)
                assert a.info()["keys"] == len(m) == a.n_keys and a.info()["valid_keys"] == m.valid(), label
            every = [i for i, r in enumerate(rows) if r == rows[t[0]]]          # the triple, and wherever else the set holds its key
            assert set(t) <= set(every)
            res, k = a.remove(np.array(every, np.uint32))
            assert (res.tolist(), k) == (m.remove(every)[0].tolist(), len(every)) and not res.any()
            step("every index of one key removed")
            cand = [rows[t[0]], fresh[0], rows[t[0]], rows[2 if n > 5 else 1]]
            cand_status = [0, 0, 0, m.status[2 if n > 5 else 1]]
            idx, st = a.add(*ac.row_columns(cand, cols), unique=True)
            np.testing.assert_array_equal(idx, m.add(cand, cand_status, True))
            assert idx[0] == n == idx[2] and st.tolist() == cand_status
            step("the removed key registered anew")
            res, k = a.remove(np.array([n, n, 0, len(m)], np.uint32))
            assert (res.tolist(), k) == (m.remove([n, n, 0, len(m)])[0].tolist(), 1) and res.tolist() == [0, 0, rc.WAS_REMOVED, rc.NOT_IN_RANGE]
            step("... and removed again")
            want_map, m = m.compact()
            np.testing.assert_array_equal(a.compact(), want_map)
            step("compacted")
            more = [rows[t[0]], fresh[1]]
            idx, st = a.add(*ac.row_columns(more, cols))
            np.testing.assert_array_equal(idx, m.add(more, [0, 0], False))
            step("an add behind the compact")
            assert a.removal() == {"removed_keys": 0, "live_keys": len(m), "remove_calls": 2, "compact_calls": 1}
            g = a.growth()
            assert g["relocations"] == 3 and g["add_calls"] == 2, g         # the first add moved, the compact, the add behind it
            with eng.keyset(scheme, *ac.row_columns(m.rows, cols)) as b:
                h = ac.signed_batch(scheme, 16385, 8, 900)[1]
                where = {j: [i for i, r in enumerate(m.rows) if r == h[j]] for j in range(8)}
                same_set(a, b, scheme, m.rows, [rc.items_over(scheme, m.rows, where, 64)], f"{scheme} n={n} sequence")
        eng.trim()


def test_stale_handles_and_no_ops(eng):
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rows, status, where = rc.gpu_set("single", 5)
    idx, sig, _ = rc.items_over("single", rows, where, 64)
    a = eng.keyset("single", *ac.row_columns(rows, 1))
    ref = a.verify(idx, *sig)
    before = (a.info(), a.growth(), a.removal())
    removed, n_keys = ctypes.c_size_t(99), ctypes.c_size_t(99)
    two = np.array([0, 4], np.uint32)
    assert lib.jjs_keyset_remove(a.handle, None, 0, None, ctypes.byref(removed)) == 0 and removed.value == 0
    assert lib.jjs_keyset_remove(a.handle, p(two), 0, None, None) == 0
    assert lib.jjs_keyset_remove(a.handle, None, 2, None, None) == -1, "a null index column"
    m = np.full(5, 77, np.uint32)
    assert lib.jjs_keyset_compact(a.handle, p(m), 4, None) == -1 and lib.jjs_keyset_compact(a.handle, p(m), 6, None) == -1, "map_len"
    assert lib.jjs_keyset_compact(a.handle, p(m), 5, ctypes.byref(n_keys)) == 0 and m.tolist() == [0, 1, 2, 3, 4] and n_keys.value == 5
    assert lib.jjs_keyset_compact(a.handle, None, 0, None) == 0, "every output is nullable"
    assert lib.jjs_keyset_removal(a.handle, None) == -1
    assert (a.info(), a.growth(), a.removal()) == before, "nothing was removed: nothing changed"
    for x, y in zip(a.verify(idx, *sig), ref):
        np.testing.assert_array_equal(x, y)
    # every output is nullable; every key removed: nothing to compact to
    assert lib.jjs_keyset_remove(a.handle, p(two), 2, None, None) == 0
    assert a.removal()["removed_keys"] == 2 and a.info()["valid_keys"] == before[0]["valid_keys"] - 2
    assert lib.jjs_keyset_remove(a.handle, p(np.arange(5, dtype=np.uint32)), 5, None, ctypes.byref(removed)) == 0 and removed.value == 3
    assert a.info()["valid_keys"] == 0 and a.removal()["live_keys"] == 0
    assert lib.jjs_keyset_compact(a.handle, p(m), 5, None) == -1, "no survivors: destroy the set instead"
    assert a.info()["keys"] == 5 and (a.verify(idx, *sig)[0] == 3).all()
    handle = a.handle
    a.close()
    assert lib.jjs_keyset_remove(handle, p(two), 2, None, None) == -1, "remove after destroy"
    assert lib.jjs_keyset_remove(handle, None, 0, None, None) == -1
    assert lib.jjs_keyset_compact(handle, None, 0, None) == -1
    assert lib.jjs_keyset_removal(handle, p(np.zeros(4, np.uint64))) == -1
    eng.trim()


def test_calls_under_a_concurrent_remove_and_compact():
    p = subprocess.run([sys.executable, os.path.join(HERE, "keyset_remove_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]

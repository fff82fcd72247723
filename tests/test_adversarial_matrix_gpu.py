"""Every device path and input format on the adversarial battery of tests/adversarial_matrix_cases.py (edge cases, the
torsion grid, coinciding points, exact equations with torsion, two faults in one item), product library.  Every cell checks
every status and the tally against the C oracle (for wire inputs: against the decode model of the cases module) and the
path_stats / info() counter that proves the path was taken:

  natural size      ext and wire, resident and host buffers (affine exists in test_gpu_parity.py; here only its new classes)
  key tables, wide  the battery tiled to the smallest multiple at or above 65 536 items (32 768 for the schemes with two
                    lookups): every key repeats 128 times or more; resident in the three formats, host buffers in affine
  ... narrow        the battery beside filler keys, so that the engine's own decision is the narrow windows
  memo              three calls in one slot: the tiled battery, the same items rotated, half the keys replaced by twins
  stale pool        a call of valid keys fills the slot's pool, then the battery, whose invalid keys get no tables
  key sets          the battery's distinct keys registered (affine; wire and ext once): key_status, by index in the latency
                    variant and in the large one with signatures of the three formats, and by key
  verify_all        Engine.verify_all and KeySet.verify_all on the whole battery from host buffers
  profiling build   tests/adversarial_matrix_child.py: forced narrow windows, the caller's order, no key arena, the verdict
                    algorithm and the forced per-item route

The memo and the stale-pool cells run at the smallest multiple of the battery ABOVE 131 072 items, not at 65 536: up to
131 072 items a call takes one of three medium slots in turn (csrc/engine_state.h pick_slot), so consecutive calls of that
size would each meet another slot's empty memo and pool; above it, calls that follow each other on one stream stay in one
big slot.  That is the smallest size at which these two cells exist."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adversarial_matrix_cases as amc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMES = list(amc.SCHEMES)
FORMATS = list(amc.FORMATS)
KT_LEAST = {"single": 65536, "double": 32768, "vargen": 32768}     # csrc/verify_job.h KT_MIN_ITEMS, KT_MIN_ITEMS_TWO_LOOKUPS
ONE_SLOT_LEAST = 131072 + 1                                        # csrc/engine_state.h MEDIUM_SLOT_ITEMS + 1
TWO_RANGES_LEAST = 65536 + 32768                                   # csrc/host_calls.h HOST_LEAD_ITEMS and half of it
KEYSET_LARGE_LEAST = 16384 + 1                                     # csrc/keyset.h KEYSET_SMALL_MAX_ITEMS + 1
NOT_IN_SET = 6


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tally_of(want):
    return [int((want == k).sum()) for k in range(4)]


def same(st, want, what):
    bad = np.nonzero(np.asarray(st) != want)[0]
    assert not len(bad), (what, len(bad), bad[:8].tolist(), np.asarray(st)[bad[:8]].tolist(), want[bad[:8]].tolist())


def run(eng, scheme, fmt, where, b, want, path):
    """One inline call: b the arrays of Forms.arrays(fmt), `where` "resident" (device pointers) or "host" (the blocking
    host-buffer call); every status, the tally, and path_stats()[path] up by one."""
    import torch
    call = {"affine": eng.verify, "ext": eng.verify_ext, "wire": eng.verify_wire}[fmt]
    args = [dev(a) for a in b] if where == "resident" else [np.ascontiguousarray(a) for a in b]
    torch.cuda.synchronize()
    before = eng.path_stats()
    st, tally = call(scheme, *args)
    if where == "resident":
        st, tally = st.cpu().numpy(), tally.cpu().numpy()
    after = eng.path_stats()
    same(st, want, (scheme, fmt, where, path))
    assert list(map(int, tally)) == tally_of(want), (scheme, fmt, where)
    assert after[path] == before[path] + 1, (scheme, fmt, where, path, before, after)


def tiled_to(f, fmt, least, want=None):
    want = f.want(fmt) if want is None else want
    return amc.tiled(f.arrays(fmt), want, amc.reps_for(f.n, least))


# ---- natural size ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["ext", "wire"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_natural_size_ext_and_wire(eng, scheme, fmt):
    f = amc.forms(scheme)
    run(eng, scheme, fmt, "resident", f.arrays(fmt), f.want(fmt), "latency")
    run(eng, scheme, fmt, "host", f.arrays(fmt), f.want(fmt), "lane_calls")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_natural_size_affine_new_classes(eng, scheme):
    rows = amc.class_rows(scheme, "exact", "precedence")
    f = amc.forms(scheme)
    b = [a[rows] for a in f.arrays("affine")]
    run(eng, scheme, "affine", "resident", b, f.want()[rows], "latency")
    run(eng, scheme, "affine", "host", b, f.want()[rows], "lane_calls")


# ---- transient key tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_tables_wide(eng, scheme, fmt):
    f = amc.forms(scheme)
    b, want = tiled_to(f, fmt, KT_LEAST[scheme])
    assert len(want) - f.n < KT_LEAST[scheme] <= len(want) and len(want) >= 128 * f.n
    run(eng, scheme, fmt, "resident", b, want, "key_tables_wide")
    if fmt == "affine":
        # the piece-by-piece host pipeline (csrc/host_calls.h plan_pieces).  At the smallest size the plan has one range of the
        # key and hash columns: the first takes 65 536 items and a rest below 32 768 joins it (u travels behind them when the
        # key tables apply).  TWO_RANGES_LEAST is the smallest size with two such ranges, every one of those columns in both;
        # tests/adversarial_matrix_child.py reads the number of pieces of both calls
        run(eng, scheme, fmt, "host", b, want, "key_tables_wide")
        run(eng, scheme, fmt, "host", *tiled_to(f, fmt, TWO_RANGES_LEAST), "key_tables_wide")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_tables_narrow_by_the_engine_s_own_decision(eng, scheme, fmt):
    f = amc.narrow_forms(scheme)
    b, want = tiled_to(f, fmt, KT_LEAST[scheme])
    n = len(want)
    keys = amc.wire_key_columns(b[1]) if fmt == "wire" else [np.tile(c, (n // f.n, 1)) for c in f.key_arrays("affine")]
    assert all(n < 128 * d and 16 * d <= n for d in amc.distinct_keys(keys)), (n, amc.distinct_keys(keys))
    run(eng, scheme, fmt, "resident", b, want, "key_tables_narrow")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_memo_three_calls_in_one_slot(eng, scheme):
    """The second call finds every key in the slot's memo, on other lanes (the items rotated by one position); the third finds
    half of them and their twins beside them -- the same prime-order part, other bytes, the validity flipped (by the Python
    oracle's point_is_valid on both): a memo that took a twin for its original would hand it the original's flags and tables.
    NOT checked here: how many keys hit (the product library has no counter; tests/adversarial_matrix_child.py holds the
    hits of this sequence against the profiling build's)."""
    f = amc.forms(scheme)
    tf, made, flipped = amc.twin_forms(scheme)
    assert made >= 60 and flipped == made
    first, want = tiled_to(f, "affine", ONE_SLOT_LEAST)
    # every tile rotated by one position (the tiles are equal, so this is the whole batch rolled by one item): each key's
    # items, and the item that stands for the key, move to the next lane
    reps = len(want) // f.n
    rotated, want_rotated = amc.tiled([np.roll(a, 1, axis=0) for a in f.arrays("affine")], np.roll(f.want(), 1), reps)
    assert all((r == np.roll(a, 1, axis=0)).all() for r, a in zip(rotated, first))
    twins, want_twins = tiled_to(tf, "affine", ONE_SLOT_LEAST)
    eng.trim()
    for b, w in ((first, want), (rotated, want_rotated), (twins, want_twins)):
        run(eng, scheme, "affine", "resident", b, w, "key_tables_wide")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_stale_pool_under_the_tables_invalid_keys_never_get(eng, scheme):
    """kt_finish_item adds table entries for invalid keys too, from pool indices whose tables were never built
    (ADVICE.md): after a call of valid keys has filled the pool those indices hold another call's valid tables, and every
    status must still be the oracle's."""
    f = amc.forms(scheme)
    b, want = tiled_to(f, "affine", ONE_SLOT_LEAST)
    reps = len(want) // f.n
    other = amc.valid_only(scheme, f.n)
    fill, fill_want = amc.tiled([other[k] for k in amc.ARG_ORDER[scheme]], np.zeros(f.n, np.uint8), reps)
    eng.trim()
    run(eng, scheme, "affine", "resident", fill, fill_want, "key_tables_wide")
    run(eng, scheme, "affine", "resident", b, want, "key_tables_wide")


# ---- registered key sets ----------------------------------------------------------------------------------------------------------
def keyset_call(ks, where, idx, sigs, fmt, want, counter, what):
    import torch
    torch.cuda.synchronize()
    before = ks.info()
    if where == "resident":
        st, tally = ks.verify(dev(idx), *[dev(c) for c in sigs], fmt=fmt)
        st, tally = st.cpu().numpy(), tally.cpu().numpy()
    else:
        st, tally = ks.verify(idx, *sigs, fmt=fmt)
    after = ks.info()
    same(st, want, what)
    assert list(map(int, tally)) == tally_of(want), what
    other = "large_calls" if counter == "small_calls" else "small_calls"
    assert after[counter] == before[counter] + 1 and after[other] == before[other], (what, before, after)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_set_registered_affine(eng, scheme):
    f = amc.forms(scheme)
    keys, idx, first = amc.registered(scheme, f, "affine")
    with eng.keyset(scheme, *keys) as ks:
        np.testing.assert_array_equal(ks.key_status, amc.key_status_reference(scheme, f, "affine", first))
        assert set(ks.key_status.tolist()) == {0, 1, 3}
        reps = amc.reps_for(f.n, KEYSET_LARGE_LEAST)
        assert (reps - 1) * f.n < KEYSET_LARGE_LEAST
        for fmt in FORMATS:
            want = f.want("affine", fmt)
            keyset_call(ks, "resident", idx, f.sig_arrays(fmt), fmt, want, "small_calls", (scheme, fmt, "latency variant"))
            keyset_call(ks, "host", idx, f.sig_arrays(fmt), fmt, want, "small_calls", (scheme, fmt, "latency variant, host"))
            big, want_big = amc.tiled(f.sig_arrays(fmt), want, reps)
            keyset_call(ks, "resident", np.tile(idx, reps), big, fmt, want_big, "large_calls", (scheme, fmt, "large variant"))
        # by key: host buffers are a drop-in for the inline call; on the device an item whose key is malformed finds nothing
        # (such a key has no canonical bytes: csrc/keyset_lookup.h) and gets NOT_IN_SET, in no tally word
        want = f.want("affine")
        before = ks.info()
        st, tally, found = ks.verify_keys(f.key_arrays("affine"), *f.sig_arrays("affine"), want_idx=True)
        same(st, want, (scheme, "by key, host"))
        assert list(map(int, tally)) == tally_of(want)
        malformed = np.any([amc.non_canonical_rows(c) for c in f.key_arrays("affine")], axis=0)
        assert malformed.any() and (found[~malformed] != ks.MISS).all() and (found[malformed] == ks.MISS).all()
        for k, col in zip(keys, f.key_arrays("affine")):
            assert (k[found[~malformed]] == col[~malformed]).all()
        mid = ks.info()
        assert mid["small_calls"] == before["small_calls"] + 1 and mid["large_calls"] == before["large_calls"], (before, mid)
        st, tally = ks.verify_keys([dev(c) for c in f.key_arrays("affine")], *[dev(c) for c in f.sig_arrays("affine")])
        st, tally = st.cpu().numpy(), tally.cpu().numpy()
        want_dev = np.where(malformed, NOT_IN_SET, want).astype(np.uint8)
        same(st, want_dev, (scheme, "by key, resident"))
        assert list(map(int, tally)) == tally_of(want_dev)
        after = ks.info()
        assert after["small_calls"] == before["small_calls"] + 2 and after["large_calls"] == before["large_calls"], (before, after)
        assert after["window_bits"] == 6 and after["keys"] == len(keys[0])


@pytest.mark.parametrize("fmt", ["ext", "wire"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_set_registered_ext_and_wire(eng, scheme, fmt):
    f = amc.forms(scheme)
    keys, idx, first = amc.registered(scheme, f, fmt)
    with eng.keyset(scheme, *keys, fmt=fmt) as ks:
        np.testing.assert_array_equal(ks.key_status, amc.key_status_reference(scheme, f, fmt, first))
        assert set(ks.key_status.tolist()) == {0, 1, 3}
        keyset_call(ks, "resident", idx, f.sig_arrays(fmt), fmt, f.want(fmt), "small_calls", (scheme, fmt, "registered in " + fmt))
        keyset_call(ks, "host", idx, f.sig_arrays("affine"), "affine", f.want(fmt, "affine"), "small_calls", (scheme, fmt, "affine signatures"))


# ---- one verdict for the batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_verify_all_on_the_whole_battery(eng, scheme):
    """The product takes the per-item route at every size (VERDICT_MIN_ITEMS is SIZE_MAX): a host-lane call for the inline
    keys, the set's latency variant for registered ones.  The forced verdict algorithm: tests/adversarial_matrix_child.py."""
    f = amc.forms(scheme)
    want = f.want()
    before = eng.path_stats()
    ok, st = eng.verify_all(scheme, *f.arrays("affine"))
    assert ok is False and st.tobytes() == want.tobytes()
    assert eng.path_stats()["lane_calls"] == before["lane_calls"] + 1
    keys, idx, _ = amc.registered(scheme, f, "affine")
    with eng.keyset(scheme, *keys) as ks:
        ok, st = ks.verify_all(idx, *f.sig_arrays("affine"))
        assert ok is False and st.tobytes() == want.tobytes()
        info = ks.info()
        assert info["small_calls"] == 1 and info["large_calls"] == 0, info
    good = amc.valid_only(scheme, f.n)
    assert eng.verify_all(scheme, *[good[k] for k in amc.ARG_ORDER[scheme]]) == (True, None)


# ---- the profiling build ------------------------------------------------------------------------------------------------------------
def test_forced_paths_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(HERE, "adversarial_matrix_child.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-4000:]

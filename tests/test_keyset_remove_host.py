"""csrc/keyset_remove.h on the CPU (tests/hostbuild/keyset_remove_harness.cpp runs the device's stage bodies, the lanes of a
launch one after the other, forwards and backwards) against the list-and-dict model of keyset_remove_cases.py: the answers and
the counts of a remove, the flag bytes, every surviving key found at the lowest index of its row, the lookup table's
invariants, adds that follow a remove, and the compaction's map, rows, flags, lookups and table words."""
import numpy as np
import pytest

import keyset_lookup_cases as kc
import keyset_remove_cases as rc
import keyset_remove_hostlib as hl

SCHEMES = ["single", "double", "vargen"]


def session(n, cols, cap=None, tables=False):
    rows, status = rc.host_set(n, cols)
    m = rc.Model(rows, status)
    return hl.Session(rows, m.flags(), cols, cap=cap, tables=tables), m


def check_set(s, m, label):
    """The session is the model: flag bytes, every row of the model found where the dict says, and the table's invariants."""
    flags, slots, rows = s.state()
    assert s.n == len(m) and rows == m.rows, label
    for c in range(s.cols):
        np.testing.assert_array_equal(flags[c], m.flags(), err_msg=f"{label} flags of column {c}")
    queries = list(dict.fromkeys(m.rows))
    np.testing.assert_array_equal(s.find(queries), m.find(queries), err_msg=f"{label} find")
    # every id that is neither removed nor malformed is found, and at the lowest index of its row
    live = [i for i in range(len(m)) if not m.removed[i] and m.status[i] != 3]
    got = s.find([m.rows[i] for i in live])
    assert all(g <= i and m.rows[g] == m.rows[i] and not m.removed[g] for g, i in zip(got.tolist(), live)), label
    assert len(slots) == kc.slot_count(len(m))
    taken = int((slots != kc.EMPTY).sum())
    assert taken <= len(slots) // 2, f"{label}: {taken} of {len(slots)} slots taken"       # so every probe sequence ends at an empty slot
    ids = slots[(slots != kc.EMPTY) & (slots != 0xFFFFFFFD)]
    assert len(set(ids.tolist())) == len(ids) and all(not m.removed[i] and m.status[i] != 3 for i in ids.tolist()), f"{label}: a live slot holds a dead id"
    return slots


@pytest.mark.parametrize("n", rc.HOST_COUNTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_remove_against_the_model(scheme, n):
    cols = rc.COLS[scheme]
    for name, idx in rc.patterns(n):
        label = f"{scheme} n={n} {name}"
        out = []
        for backwards in (False, True):
            s, m = session(n, cols)
            want, n_removed, n_valid = m.remove(idx)
            got, counts = s.remove(idx, backwards)
            np.testing.assert_array_equal(got, want, err_msg=label)
            assert counts == [n_removed, n_valid], label
            slots = check_set(s, m, label)
            out.append((s.state()[0].tobytes(), (slots == 0xFFFFFFFD).tobytes()))
            # again: everything was removed already, nothing changes
            again, counts = s.remove(idx, backwards)
            np.testing.assert_array_equal(again, m.remove(idx)[0], err_msg=f"{label} again")
            assert counts == [0, 0] and set(again.tolist()) <= {rc.WAS_REMOVED, rc.NOT_IN_RANGE}
            check_set(s, m, f"{label} again")
            s.close()
        assert out[0] == out[1], f"{label}: the lanes' order shows"


@pytest.mark.parametrize("n", (3, 4, 5, 257))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_adds_after_a_remove(scheme, n):
    """A removed key offered again: UNIQUE registers it anew at a new index (or answers with the lowest surviving duplicate);
    APPEND registers whatever it is given.  4 -> 5 keys is the 8-to-16 slot step: the rebuilt table skips the removed ids."""
    cols = rc.COLS[scheme]
    t = rc.triple(n)
    for name, idx in (("lowest_of_three", [t[0]]), ("all_of_three", list(t)), ("first_and_last", [0, n - 1])):
        for unique in (True, False):
            label = f"{scheme} n={n} {name} unique={unique}"
            s, m = session(n, cols, cap=n + 8)
            s.remove(np.array(idx, np.uint32)); m.remove(idx)
            rng = np.random.default_rng(n)
            fresh = kc.rand_row(rng, cols)
            cand = [m.rows[t[0]], fresh, m.rows[t[0]], m.rows[-2], fresh, kc.rand_row(rng, cols)]
            status = [0, 0, 0, m.status[-2], 0, 3]
            want = m.add(cand, status, unique)
            got = s.add(cand, [rc.FLAG_OF_STATUS[x] for x in status], unique)
            np.testing.assert_array_equal(got, want, err_msg=label)
            if unique and name == "all_of_three":
                assert got[0] == n == got[2], "registered anew, once"
            check_set(s, m, label)
            # ... and the new index can be removed in turn: the triple's key is then found at its next survivor, or nowhere
            s.remove(got[:1]); m.remove(got[:1])
            check_set(s, m, f"{label}, removed again")
            s.close()


@pytest.mark.parametrize("n", rc.HOST_COUNTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_compact_against_the_model(scheme, n):
    cols = rc.COLS[scheme]
    for name, idx in rc.patterns(n):
        label = f"{scheme} n={n} {name}"
        tables = n <= 5 or (n == 257 and scheme != "double" and name in ("every_second", "across_a_block_edge"))
        for backwards in (False, True)[:1 if tables and n > 5 else 2]:
            s, m = session(n, cols, tables=tables)
            s.remove(idx); m.remove(idx)
            want_map, after = m.compact()
            got_map, n_new = s.compact(backwards)
            if len(after) == 0:
                assert n_new == -1, label
                s.close()
                continue
            assert n_new == len(after) == s.n, label
            np.testing.assert_array_equal(got_map, want_map, err_msg=label)
            check_set(s, after, label)
            assert not (s.state()[1] == 0xFFFFFFFD).any(), "a table built from empty"
            if tables:
                src = np.flatnonzero(want_map != rc.GONE)
                for new in sorted({0, len(src) // 2, len(src) - 1}):         # the whole 204 KB of the first, a middle and the last survivor
                    for c in range(cols):
                        np.testing.assert_array_equal(s.table(c, new), hl.pattern_table(c, int(src[new])), err_msg=f"{label} table {new}")
            s.close()


def test_the_scan_spans_the_blocks_of_a_compaction():
    """1 300 keys, every third removed, then all below 1 290: whole blocks without a survivor ahead of the ranks."""
    s, m = session(1300, 1)
    for idx in (np.arange(0, 1300, 3), np.arange(1, 1290)):
        s.remove(idx.astype(np.uint32)); m.remove(idx)
    want_map, after = m.compact()
    got_map, n_new = s.compact()
    assert n_new == len(after) == 6
    np.testing.assert_array_equal(got_map, want_map)
    check_set(s, after, "two removes, then compact")
    s.close()

"""The CPU build of csrc/keyset_add.h (adding keys to a live key set): the stage bodies the device runs -- probe, claim, mark,
scan, gather, answers, the ranged insert into the set's lookup table -- against the Python dict of JJS_KEYSET_ADD_UNIQUE and the
list of JJS_KEYSET_ADD_APPEND (keyset_add_cases.py), for every scheme and key format, at 1, 255, 256, 257 and 65 537
candidates: the block edge and the edge of the 256 x 256 two-level scan -- and over a list of 1 300 candidates whose 300 new
keys first occur in every wave and in at least five blocks.  The harness runs the stage bodies lane by lane; the block count, the combine of
the scan lanes' totals and the rank inside a block are the kernels' own code (keyset_add_kernels.h), which the same lists check on
the device (tests/test_keyset_add_gpu.py).  No GPU."""
import numpy as np
import pytest

import keyset_add_cases as ac
import keyset_add_hostlib as ka
import keyset_lookup_cases as kc

SCHEMES = ["single", "double", "vargen"]
FMTS = ["affine", "ext", "wire"]


def run(scheme, fmt, n, unique, encs=None):
    held, bad = ac.base_set(scheme)
    encs = encs or ac.candidates(scheme, fmt, n)
    rows = [ac.canonical_row(e, fmt) for e in encs]
    got = ka.add(ac.row_columns(held, ac.COLS[scheme]), bad, kc.FORMATS[fmt], ac.columns(encs, scheme, fmt), unique)
    return held, bad, rows, got


def check_lookup(got, held_after, bad_after):
    """The table after the add is the table of a fresh build, slot for slot (the CPU build inserts in the order of the ids, so
    a fresh build is deterministic), and as a map: the lowest index of every canonical key, and nothing else."""
    np.testing.assert_array_equal(got["slots"], got["fresh"])
    assert len(got["slots"]) == kc.slot_count(len(held_after))
    affine, _ = kc.model(held_after, bad_after)
    assert sorted(s for s in got["slots"].tolist() if s != kc.EMPTY) == sorted(affine.values())


def spread_of_first_occurrences(want_idx, n_old):
    """(blocks of 256 candidates, waves inside a block) that hold a first occurrence."""
    seen, at = set(), []
    for i, x in enumerate(want_idx.tolist()):
        if x != ac.MISS and x >= n_old and x not in seen:
            seen.add(x); at.append(i)
    return {i // 256 for i in at}, {(i % 256) // 64 for i in at}


@pytest.mark.parametrize("n", ac.COUNTS + (0,))
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_unique_against_the_dict(scheme, fmt, n):
    """n = 0: the spread list -- 1 300 candidates, 300 distinct new keys among them, first occurrences in every wave and in
    five blocks or six: the block bases of the scan and the ranks inside a block carry values other than zero, and the new keys are more
    than one block."""
    spread = n == 0
    held, bad, rows, got = run(scheme, fmt, n, True, ac.spread_candidates(scheme, fmt) if spread else None)
    want_idx, new, known = ac.unique_model(held, bad, rows)
    if spread:
        blocks, waves = spread_of_first_occurrences(want_idx, len(held))
        assert len(rows) == ac.SPREAD_N and blocks >= set(range(5)) and waves == {0, 1, 2, 3} and len(new) > 256 + 6
    if n >= 255 or spread:      # what the lists are about
        assert known > 0 and len(new) >= 6 and (want_idx == ac.MISS).any() and (want_idx == 1).any() and not (want_idx == 4).any()
        assert any(ac.row_status(r) == 1 for r in new), "an off-curve point or Z = 0 is registered, status 1"
    np.testing.assert_array_equal(got["idx"], want_idx)
    assert got["n_added"] == len(new)
    cols = ac.COLS[scheme]
    after = [b"".join(got["rows"][c][i].tobytes() for c in range(cols)) for i in range(len(held) + len(new))]
    assert after == held + new, "the old rows untouched, the first occurrences behind them in input order"
    want_status = [3 if r is None else ac.row_status(r) for r in rows]
    assert got["status"].tolist() == want_status
    for i, r in enumerate(new):
        f = [int(got["flags"][c][len(held) + i]) for c in range(cols)]
        assert all(not (x & 1) for x in f) and (all(x & 2 for x in f)) == (ac.row_status(r) == 0), (i, f)      # KT_KEY_MALFORMED 1, KT_KEY_VALID 2
    check_lookup(got, held + new, bad + [0] * len(new))
    assert got["rebuilt"] == (kc.slot_count(len(held) + len(new)) != kc.slot_count(len(held)))


@pytest.mark.parametrize("n", ac.COUNTS + (0,))
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_append_against_the_list(scheme, fmt, n):
    """n = 0: the spread list of the UNIQUE test, appended."""
    held, bad, rows, got = run(scheme, fmt, n, False, ac.spread_candidates(scheme, fmt) if n == 0 else None)
    n = len(rows)
    assert got["n_added"] == n and got["idx"].tolist() == list(range(len(held), len(held) + n))
    assert got["status"].tolist() == [3 if r is None else ac.row_status(r) for r in rows]
    cols = ac.COLS[scheme]
    after = [b"".join(got["rows"][c][i].tobytes() for c in range(cols)) for i in range(len(held) + n)]
    assert after[:len(held)] == held
    for i, r in enumerate(rows):
        assert r is None or after[len(held) + i] == r, i
    # a malformed candidate is registered all the same: whatever its row holds, nothing finds it
    stand_in = [r if r is not None else after[len(held) + i] for i, r in enumerate(rows)]
    check_lookup(got, held + stand_in, bad + [int(r is None) for r in rows])


def test_one_new_key_goes_into_the_table_in_place_and_nine_need_more_slots():
    held, bad, rows, got = run("single", "affine", 1, True)
    assert got["n_added"] == 1 and not got["rebuilt"] and len(got["slots"]) == 16
    held, bad, rows, got = run("single", "affine", 255, True)
    assert len(held) + got["n_added"] > 8 and got["rebuilt"] and len(got["slots"]) == 32


def test_the_scan_of_the_block_counts_at_its_edges():
    """One lane of 256 takes ceil(blocks / 256) counts: 255, 256 and 257 blocks (one count per lane, then two for some), 65 535
    .. 65 537 (2^24 candidates are 65 536 blocks: 256 counts per lane), and counts that are all 256 (every candidate new)."""
    rng = np.random.default_rng(8)
    for blocks in (1, 2, 255, 256, 257, 511, 512, 513, 1000, 65535, 65536, 65537):
        for counts in (rng.integers(0, 257, blocks), np.full(blocks, 256), np.zeros(blocks, np.int64)):
            got, total = ka.scan(counts)
            want = np.concatenate([[0], np.cumsum(counts)[:-1]])
            np.testing.assert_array_equal(got, want.astype(np.uint32), err_msg=f"blocks={blocks}")
            assert total == int(np.sum(counts))

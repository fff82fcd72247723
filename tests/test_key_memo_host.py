"""The memo of a slot's last key-table call (csrc/key_tables.h step 5) on the CPU build: sequences of calls in one slot give
the C oracle's statuses whatever the memo holds, and hit exactly the keys they share with the call before (MemoModel)."""
import numpy as np
import pytest

from key_memo_cases import MemoModel, expected, sequences
import key_memo_hostlib as mh

SCHEMES = ["single", "double", "vargen"]


@pytest.fixture(scope="module")
def cases():
    return {s: sequences(s, n_keys=8, per_key=3) for s in SCHEMES}


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sequences_in_one_slot(scheme, cases):
    want = {}
    for name, steps in cases[scheme].items():
        slot, model = mh.Slot(cap=64), MemoModel()
        try:
            seen_hit = False
            for k, (b, window, flags) in enumerate(steps):
                if "new_pool" in flags:
                    slot.new_pool(); model.flush()
                st, hits, built = slot.call(scheme, b, window, off="off" in flags)
                want_hits, want_built = model.call(scheme, b, window, off="off" in flags)
                print(scheme, name, k, "hits", hits, "built", built)
                assert (hits, built) == (want_hits, want_built), (name, k)
                seen_hit = seen_hit or sum(hits) > 0
                if not window:
                    continue
                if id(b) not in want:
                    want[id(b)] = (b, expected(scheme, b))
                assert st.tolist() == want[id(b)][1].tolist(), (name, k)
            assert seen_hit == (name != "disjoint sets"), name        # every other sequence makes the memo engage
        finally:
            slot.close()


def test_pool_indices_run_out_only_with_the_pool():
    """As many distinct keys as the pool holds, then as many others: every miss finds an index no hit holds."""
    from key_memo_cases import by_keys, pool_of_items
    a, _ = pool_of_items("single", 8, 2, 7)
    b, _ = pool_of_items("single", 8, 2, 8)
    keys = lambda x: len(set(map(bytes, x["PK"])))     # noqa: E731
    slot = mh.Slot(cap=max(keys(a), keys(b)))
    try:
        for batch in (a, b, by_keys(a, 8, range(4)), a):
            st, _, _ = slot.call("single", batch, 5)
            assert st.tolist() == expected("single", batch).tolist()
    finally:
        slot.close()

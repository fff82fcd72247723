"""The CPU build of csrc/keyset_lookup.h (key sets by key): the insert and probe functions the device runs, against a
Python dict (lowest index per canonical key) and a Python restatement of the hash, over crafted sets -- and the by-key
verification of a mixed batch per scheme against the oracle.  No GPU."""
import numpy as np
import pytest

import jjs_oracle as o
import keyset_lookup_cases as kc
import keyset_lookup_hostlib as kl
from helpers import IDENT, fe_bytes, make_batch, oracle_verify

CASES = kc.lookup_cases()
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}


def test_the_slot_count_is_the_power_of_two_from_twice_the_keys_and_at_least_eight():
    for n in (1, 2, 3, 4, 5, 8, 9, 64, 65, 1000, 1 << 15, (1 << 15) + 1, 1 << 24):
        assert kl.slot_count(n) == kc.slot_count(n), n
    assert [kl.slot_count(n) for n in (1, 4, 5, 8, 9, 64)] == [8, 8, 16, 16, 32, 128]


def test_the_hash_is_the_python_restatement():
    rng = np.random.default_rng(3)
    for cols in (1, 2):
        for seed in (0, 1, 0xFFFFFFFFFFFFFFFF, int(rng.integers(0, 1 << 63))):
            for _ in range(16):
                row = rng.bytes(64 * cols)          # any bytes: bit 255 of v is REPLACED by the parity of u
                assert kl.hash_affine(row, seed) == kc.kl_hash(row, seed)
    # the encoding words, not the affine bytes: u enters by its parity alone
    a = bytearray(kc.rand_row(rng, 1)); b = bytearray(a); b[5] ^= 0x40; c = bytearray(a); c[0] ^= 1
    assert kl.hash_affine(bytes(a), 0) == kl.hash_affine(bytes(b), 0) != kl.hash_affine(bytes(c), 0)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_lookup_against_the_dict(c):
    keys, queries = kc.columns(c)
    bad = np.array(c["bad"], np.uint8) if c["bad"] is not None else None
    for order in (c["orders"] or [None]):
        idx, slots, _ = kl.find(keys, kc.FORMATS[c["fmt"]], queries, bad=bad, order=order)
        np.testing.assert_array_equal(idx, c["want"], err_msg=f"{c['name']} order={order}")
        assert len(slots) == kc.slot_count(len(c["keys"]))
        if c["slots"] is not None and order is None:
            assert slots.tolist() == [kc.EMPTY if s is None else s for s in c["slots"]], c["name"]
        # every entry is the lowest index of its key, and nothing else is in the table
        affine, _ = kc.model(c["keys"], c["bad"])
        assert sorted(s for s in slots.tolist() if s != kc.EMPTY) == sorted(affine.values()), c["name"]


def test_an_encoding_that_did_not_decode_at_registration_is_never_hit():
    rng = np.random.default_rng(5)
    rows = [kc.rand_row(rng, 1) for _ in range(6)]
    keys = [np.frombuffer(b"".join(rows), np.uint8).reshape(6, 64), None]
    bad = np.array([0, 0, 1, 0, 0, 0], np.uint8)
    idx, _, on_curve = kl.find(keys, 0, keys, bad=bad)
    assert idx.tolist() == [0, 1, kc.MISS, 3, 4, 5] and not on_curve.any()


def test_a_seed_moves_the_keys_and_changes_no_answer():
    c = next(c for c in CASES if c["name"] == "chain1")
    keys, queries = kc.columns(c)
    tables = []
    for seed in (0, 1, 0x123456789ABCDEF):
        idx, slots, _ = kl.find(keys, 0, queries, seed=seed)
        np.testing.assert_array_equal(idx, c["want"])
        tables.append(slots.tolist())
    assert tables[0] != tables[1] != tables[2]


def mixed_batch(scheme):
    """96 items over 12 keys of which 8 are registered, beside a registered identity (not `is_valid`) and a registered key with
    u = q (malformed: never found).  Returns (batch, the set's columns, the index every item must be found at or MISS)."""
    b = make_batch(scheme, 96, seed=21, n_keys=12)
    names = KEYCOLS[scheme]
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in names], 1))
    uniq, counts = np.unique(cat, axis=0, return_counts=True)
    assert len(uniq) >= 10
    reg = uniq[np.argsort(-counts, kind="stable")[:8]]           # eight of the twelve honest keys
    ident = reg[:1].copy(); ident[0, :64] = IDENT
    nc = reg[:1].copy(); nc[0, :32] = fe_bytes(o.Q)
    reg = np.concatenate([reg, ident, nc])
    invalid_items, bad_items = np.arange(5, 96, 19), np.arange(3, 96, 17)
    cat[invalid_items] = reg[8]
    cat[bad_items] = reg[9]
    for i, name in enumerate(names):
        b[name] = np.ascontiguousarray(cat[:, 64 * i:64 * i + 64])
    found = kc.want([r.tobytes() for r in reg], "affine", [r.tobytes() for r in cat])
    assert (found[invalid_items] == 8).all() and (found[bad_items] == kc.MISS).all()
    keys = [np.ascontiguousarray(reg[:, 64 * i:64 * i + 64]) for i in range(len(names))]
    return b, keys, found


@pytest.mark.parametrize("scheme", ["single", "double", "vargen"])
def test_by_key_verification_of_a_mixed_batch(scheme):
    b, keys, found = mixed_batch(scheme)
    want = oracle_verify(scheme, b)
    miss = found == kc.MISS
    assert miss.sum() >= 10 and (~miss).sum() >= 40 and (want[found == 8] == 1).all() and len(set(want[~miss].tolist())) >= 3
    want_by_key = np.where(miss, 6, want).astype(np.uint8)
    for positions in (0, 4, 8, 16):
        st, tally, idx = kl.verify_keys(scheme, keys, [b[k] for k in KEYCOLS[scheme]], b["u"], b["R"], b.get("Rp"), b["m"], positions)
        np.testing.assert_array_equal(idx, found, err_msg=f"positions={positions}")
        np.testing.assert_array_equal(st, want_by_key, err_msg=f"positions={positions}")
        assert tally.tolist() == [int((want[~miss] == k).sum()) for k in range(4)] and int(tally.sum()) == 96 - int(miss.sum())

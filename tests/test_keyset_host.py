"""The CPU build of csrc/keyset.h (registered key sets) against the oracle: both variants -- one lane per item, and the
latency variant's 4, 8 or 16 lanes per equation -- for the three schemes, with invalid and malformed keys and indices
beyond the set.  No GPU."""
import numpy as np
import pytest

import jjs_oracle as o
import keyset_hostlib as kh
from helpers import IDENT, edge_cases, fe_bytes, make_batch, oracle_verify, torsion_grid

KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
SCHEMES = ["single", "double", "vargen"]
VARIANTS = [0, 4, 8, 16]


def register(scheme, b):
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in KEYCOLS[scheme]], 1))
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    return [uniq[:, 64 * i:64 * i + 64] for i in range(len(KEYCOLS[scheme]))], inv.reshape(-1).astype(np.uint32)


def run(scheme, b, keys, idx, positions):
    return kh.verify(scheme, keys, idx, b["u"], b["R"], b.get("Rp"), b["m"], positions)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_mixed_batch_over_eight_keys_with_invalid_and_malformed_ones(scheme):
    b = make_batch(scheme, 96, seed=21, n_keys=8)
    keys, idx = register(scheme, b)
    # two more keys: the identity (not `is_valid`) and one with a coordinate that is not canonical (u = q), a few items each
    ident = keys[0][:1].copy(); ident[0] = IDENT
    nc = keys[0][:1].copy(); nc[0, :32] = fe_bytes(o.Q)
    keys = [np.concatenate([k, ident, nc]) if i == 0 else np.concatenate([k, k[:1], k[:1]]) for i, k in enumerate(keys)]
    bad_items, invalid_items = np.arange(3, 96, 17), np.arange(5, 96, 19)
    idx[invalid_items] = len(keys[0]) - 2
    idx[bad_items] = len(keys[0]) - 1
    for i, name in enumerate(KEYCOLS[scheme]):
        b[name] = keys[i][idx]
    want = oracle_verify(scheme, b)
    assert (want[bad_items] == 3).all() and (want[invalid_items] == 1).all()
    assert len(set(want.tolist())) >= 3
    for positions in VARIANTS:
        st, key_status = run(scheme, b, keys, idx, positions)
        np.testing.assert_array_equal(st, want, err_msg=f"positions={positions}")
    assert key_status[-1] == 3 and key_status[-2] == 1


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("source", ["edge_cases", "torsion_grid"])
def test_every_item_its_own_registered_key(scheme, source):
    b = edge_cases(scheme) if source == "edge_cases" else torsion_grid(scheme, reps=1)
    keys, idx = register(scheme, b)
    want = oracle_verify(scheme, b)
    for positions in (VARIANTS if source == "edge_cases" else [0, 8]):
        st, _ = run(scheme, b, keys, idx, positions)
        np.testing.assert_array_equal(st, want, err_msg=f"positions={positions}")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_indices_beyond_the_set_are_malformed(scheme):
    b = make_batch(scheme, 40, seed=23, n_keys=4, mix=False)
    keys, idx = register(scheme, b)
    want = oracle_verify(scheme, b)
    assert (want == 0).all()
    idx[[1, 7, 30]] = [len(keys[0]), 0xFFFFFFFF, 1 << 20]
    want[[1, 7, 30]] = 3
    for positions in VARIANTS:
        st, _ = run(scheme, b, keys, idx, positions)
        np.testing.assert_array_equal(st, want, err_msg=f"positions={positions}")

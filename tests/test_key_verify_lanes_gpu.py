"""key_verify_kernel with three waves per SIMD: digits read from LDS, sums skipped by waves without a valid key, sums started
from their top entry (csrc/key_tables.h kt_finish_item_lanes).

End to end at the smallest size at which the key-table path engages -- 65 536 single signatures over 256 keys (wide windows)
and over 2 048 keys (narrow), 32 768 double and per-item-generator signatures -- on batches made for what the kernel now
does by wave:
  * the items of a key form a run in the kernel's order (the device groups the items by their first key column), and the run
    lengths here are uneven (1, 63, 64, 65, 127, 129, ... and whatever fills the batch), so that the boundaries of waves and
    blocks fall inside runs and a wave holds several keys;
  * three keys are not valid -- the identity, the point of order 2, a point of mixed order -- with runs of 1, 64 and 200
    items: 200 items of one key fill at least two whole waves wherever the run starts (no lane with a valid key: the wave
    skips the sum), the runs of 1 and 64 share waves with valid keys (a lane of an invalid key reads the tables of a valid
    one).  For the double and the per-item-generator scheme the run of 200 has its invalid key in the SECOND key column,
    under one first key;
  * u = 0, u = r - 1 (in range, the equation fails) and u = r (malformed, also under an invalid key: malformed comes first).
The base batches, with the statuses of their own constructions (wrong key, changed message, invalid R), are those of
tests/test_affine_tables_gpu.py.  Every status is known by construction; the first 4 096 items, which hold every special
item, are held against the C oracle.

NOT added: a run over a key pool filled with 0xFF.  The engine has no hook that fills a pool through its own
allocation path, and an entry point for the test alone is not worth its surface."""
import functools

import numpy as np
import pytest

import jjs_oracle as o
from helpers import ARG_ORDER, IDENT, ORDER2, _add_order2, fe_bytes, oracle_verify
from test_affine_tables_gpu import KEYCOLS, RCOLS, SAMPLE, construct, dev

pytestmark = pytest.mark.gpu

HEAD_RUNS = (1, 63, 64, 65, 127, 129)          # the run lengths of the first 96 keys, in turn
N_HEAD = 96
INVALID_RUNS = (1, 64, 200)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


@functools.lru_cache(None)
def uneven(scheme, n_base, n_keys, seed, n_total, rot):
    """-> (batch of n_total items, statuses).  `rot` turns which invalid point gets which run length."""
    base, base_want = construct(scheme, n_base, n_keys, seed)
    cols = KEYCOLS[scheme] + RCOLS[scheme]
    i = np.arange(n_base)
    # the base items whose first key column construct() left alone or gave another valid key: the pool the runs are drawn from
    touched = np.zeros(n_base, bool)
    for cls in (11, 13, 17):
        rows = i[i % 64 == cls]
        for j, name in enumerate(cols):
            if name in KEYCOLS[scheme]:
                touched[rows[j::len(cols)]] = True
    pool = i[~touched]
    keys, inverse = np.unique(base["PK"][pool], axis=0, return_inverse=True)
    members = [pool[inverse.reshape(-1) == k] for k in range(len(keys))]
    # keys behind the head that have items construct() left valid: they lend the items that are edited below
    good = [k for k in range(N_HEAD, len(keys)) if (base_want[members[k]] == 0).any()]
    assert len(good) >= 10
    lend = [members[k][base_want[members[k]] == 0] for k in good]

    # the special items come first (the oracle's sample holds them all), then the runs key by key
    sel, edits = [], []                  # edits: (position, column, bytes, status)
    invalid = [IDENT, ORDER2, _add_order2(keys[:1])[0]]
    invalid = invalid[rot:] + invalid[:rot]
    second = KEYCOLS[scheme][1] if len(KEYCOLS[scheme]) > 1 else None
    where = []
    for point, length in zip(invalid, INVALID_RUNS):
        # the run of 200 of a scheme with two key columns: the invalid key in the second column, all under ONE first key
        col = second if (second and length == 200) else "PK"
        where.append(col)
        donors = lend[3] if col != "PK" else np.concatenate(lend[4:10])
        for k in range(length):
            edits.append((len(sel), col, point, 1))
            sel.append(donors[k % len(donors)])
    first_of_200 = len(sel) - 200
    for k, u_val, st in ((0, 0, 2), (1, o.R_ORDER - 1, 2), (2, o.R_ORDER, 3)):
        edits.append((len(sel), "u", fe_bytes(u_val), st))
        sel.append(lend[k][0])
    # u under an invalid key: r is malformed whatever the key is; 0 is in range and the key decides
    edits.append((first_of_200, "u", fe_bytes(o.R_ORDER), 3))
    edits.append((first_of_200 + 1, "u", fe_bytes(0), 1))
    n_front = len(sel)
    assert n_front <= SAMPLE
    counts = np.array([HEAD_RUNS[k % len(HEAD_RUNS)] for k in range(N_HEAD)] + [0] * (len(keys) - N_HEAD))
    rest, tail = n_total - n_front - counts.sum(), len(keys) - N_HEAD
    counts[N_HEAD:] = rest // tail
    counts[N_HEAD:N_HEAD + rest % tail] += 1
    assert counts.sum() + n_front == n_total and counts.min() >= 1
    for k, m in enumerate(members):
        sel.extend(m[np.arange(counts[k]) % len(m)].tolist())
    sel = np.array(sel)
    b = {name: v[sel].copy() for name, v in base.items()}
    want = base_want[sel].copy()
    for pos, col, val, st in edits:
        b[col][pos] = val
        want[pos] = st
    sample = {name: v[:SAMPLE] for name, v in b.items()}
    assert (oracle_verify(scheme, sample) == want[:SAMPLE]).all(), "the construction against the C oracle"
    assert all((want == s).sum() > 0 for s in (0, 1, 2, 3))
    # what the batch was made for: uneven runs by first key, and the three invalid keys with their runs
    _, run_len = np.unique(b["PK"], axis=0, return_counts=True)
    assert set(HEAD_RUNS) <= set(run_len.tolist())
    for point, length, col in zip(invalid, INVALID_RUNS, where):
        assert (b[col] == point).all(1).sum() == length
    return b, want


def run(eng, scheme, b, want, path):
    import torch
    torch.cuda.synchronize()
    before = eng.path_stats()
    st, tally = eng.verify(scheme, *[dev(b[k]) for k in ARG_ORDER[scheme]])
    st, tally = st.cpu().numpy(), tally.cpu().numpy()
    after = eng.path_stats()
    bad = np.nonzero(st != want)[0]
    assert not len(bad), (scheme, len(bad), bad[:8].tolist(), st[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert tally.tolist() == [int((want == k).sum()) for k in range(4)]
    assert after[path] == before[path] + 1, (path, before, after)


@pytest.mark.parametrize("n_keys,path,rot", [(256, "key_tables_wide", 0), (2048, "key_tables_narrow", 1)])
def test_single_65536_items_uneven_runs_and_invalid_keys(eng, n_keys, path, rot):
    b, want = uneven("single", 8192, n_keys, 41, 65536, rot)
    run(eng, "single", b, want, path)


@pytest.mark.parametrize("scheme,rot", [("double", 2), ("vargen", 0)])
def test_double_and_vargen_32768_items_uneven_runs_and_invalid_keys(eng, scheme, rot):
    b, want = uneven(scheme, 4096, 128, 43, 32768, rot)
    run(eng, scheme, b, want, "key_tables_wide")

"""Sequences of key-table calls in ONE slot for the memo of the slot's last call (csrc/key_tables.h step 5), shared by the
CPU-build and the device tests: the batches, and what the memo must do with them.

`MemoModel` is the specification, in a dozen lines: the memo is the set of distinct key byte strings (per key column) of the
slot's last call that took the tables, valid for one window width and one column layout; a call hits exactly the keys it
shares with it.  Everything else -- a turned-down call, a wire call, a new pool -- empties it."""
import numpy as np

import jjs_oracle as o
from helpers import ARG_ORDER, edge_cases, fe_bytes, make_batch, oracle_verify

KEY_COLUMNS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}


def distinct_keys(scheme, b):
    return [set(map(bytes, np.ascontiguousarray(b[k]))) for k in KEY_COLUMNS[scheme]]


class MemoModel:
    def __init__(self):
        self.keys, self.window = None, 0

    def flush(self):
        self.keys = None

    def call(self, scheme, b, window, off=False):
        """-> (hits per column, built per column) the call must report."""
        cur = distinct_keys(scheme, b)
        if not window:
            self.keys = None
            return [0] * len(cur), [0] * len(cur)
        live = not off and self.keys is not None and self.window == window and len(self.keys) == len(cur)
        hits = [len(c & m) for c, m in zip(cur, self.keys)] if live else [0] * len(cur)
        self.keys, self.window = (None if off else cur), window
        return hits, [len(c) - h for c, h in zip(cur, hits)]


def take(b, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in b.items()}


def concat(*bs):
    return {k: np.concatenate([b[k] for b in bs]) for k in bs[0]}


def pool_of_items(scheme, n_keys, per_key, seed):
    """n_keys * per_key signed items with the usual corruptions; item i is under key i % n_keys (a corrupted item may carry
    its neighbour's key or a torsion point instead), and the hand-built edge cases of the scheme behind them: keys that are the
    identity, of order 2, of mixed order, off the curve, and with a coordinate >= q."""
    return make_batch(scheme, n_keys * per_key, seed=seed, n_keys=n_keys), edge_cases(scheme)


def by_keys(b, n_keys, want):
    """the items of pool_of_items' batch whose key index is in `want`"""
    want = np.isin(np.arange(len(b["u"])) % n_keys, list(want))
    return take(b, np.where(want)[0])


def near_twin(scheme, b):
    """b plus a copy of its first item whose key differs from it in the last byte only (63 of 64 bytes equal)"""
    t = take(b, [0])
    t["PK"] = t["PK"].copy()
    t["PK"][0, 63] ^= 1
    return concat(b, t)


def expected(scheme, b):
    return oracle_verify(scheme, b)


def sequences(scheme, n_keys=12, per_key=6, seed=41):
    """name -> list of steps; a step is (batch, window, flags) with flags a set of "off" (a wire call), "new_pool" (before it).
    Window 6 stands for >= 128 signatures per key on the device, 5 for fewer, 0 for a batch that turns the tables down."""
    base, edges = pool_of_items(scheme, n_keys, per_key, seed)
    other, _ = pool_of_items(scheme, n_keys, per_key, seed + 1)
    K = range(n_keys)
    A = concat(by_keys(base, n_keys, K), edges)
    B = by_keys(other, n_keys, K)                                   # disjoint from A
    lo, hi, mid = by_keys(base, n_keys, range(0, n_keys // 2)), by_keys(base, n_keys, range(n_keys // 2, n_keys)), \
        by_keys(base, n_keys, range(n_keys // 4, 3 * n_keys // 4))
    s = {
        "same keys three times": [(A, 6, ()), (A, 6, ()), (A, 6, ())],
        "disjoint sets": [(A, 6, ()), (B, 6, ()), (A, 6, ())],
        "half-overlapping sets": [(lo, 6, ()), (mid, 6, ()), (hi, 6, ())],
        "set, superset, subset": [(mid, 6, ()), (A, 6, ()), (lo, 6, ())],
        # hi's keys take the pool indices lo's left; lo comes back two calls later and must be rebuilt
        "a key leaves, its index is reused, it returns": [(concat(lo, edges), 6, ()), (hi, 6, ()), (concat(lo, edges), 6, ()), (A, 6, ())],
        "two keys equal in 63 bytes": [(near_twin(scheme, lo), 6, ()), (near_twin(scheme, A), 6, ()), (lo, 6, ())],
        "width 6, 5, 6": [(A, 6, ()), (A, 5, ()), (A, 5, ()), (A, 6, ())],
        "a wire call between": [(A, 6, ()), (mid, 6, ("off",)), (A, 6, ()), (A, 6, ())],
        "a new pool between": [(A, 6, ()), (A, 6, ("new_pool",)), (A, 6, ())],
        "a turned-down call between": [(A, 6, ()), (B, 0, ()), (A, 6, ()), (A, 6, ())],
    }
    if len(KEY_COLUMNS[scheme]) == 2:
        # column 0 as in A, column 1 from B's rows: one column hits while the other misses
        second = KEY_COLUMNS[scheme][1]
        n = min(len(A["u"]), len(B["u"]))
        X = take(A, range(n))
        X[second] = B[second][:n].copy()
        s["one column hits, the other misses"] = [(take(A, range(n)), 6, ()), (X, 6, ()), (take(A, range(n)), 6, ())]
    return s

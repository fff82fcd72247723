"""Removing keys from a live key set and compacting it (csrc/keyset_remove.h): the Python model every remove, add-after-remove and
compact is checked against -- a list of (row, status, removed) and, for the lookups, the dict of keyset_lookup_cases.model over
the rows that are neither removed nor malformed -- and the sets and removal patterns shared by tests/test_keyset_remove_host.py
(CPU build), tests/test_keyset_remove_gpu.py and tests/keyset_remove_child.py (device).

The host test needs no curve points (nothing there reads a row as a point): its keys are random canonical coordinates with the
flag bytes given.  The device tests take real keys with signatures from keyset_add_cases.signed_batch."""
import numpy as np

import keyset_add_cases as ac
import keyset_lookup_cases as kc

MISS = 0xFFFFFFFF
GONE = 0xFFFFFFFF
WAS_REMOVED, NOT_IN_RANGE = 8, 0xFF
MALFORMED, VALID, REMOVED = 1, 2, 4          # KT_KEY_* of csrc/key_tables.h and csrc/keyset_remove.h
FLAG_OF_STATUS = {0: VALID, 1: 0, 3: MALFORMED}
HOST_COUNTS = (1, 3, 4, 5, 255, 256, 257, 1300)      # the 8-to-16 slot step at 4 -> 5 keys; the block edge; several blocks
GPU_COUNTS = (4, 5, 257, 1300)
COLS = ac.COLS
FF_ROW = b"\xff" * 64


class Model:
    """The set as a list.  status: 0 valid, 1 not `is_valid`, 3 malformed -- as registered; a removed key reports 3."""

    def __init__(self, rows, status):
        self.rows, self.status, self.removed = list(rows), [int(s) for s in status], [False] * len(rows)

    def __len__(self):
        return len(self.rows)

    def key_status(self):
        return np.array([3 if r else s for s, r in zip(self.status, self.removed)], np.uint8)

    def flags(self):
        """The flag byte every point column of key i carries."""
        return np.array([(FLAG_OF_STATUS[s] | MALFORMED | REMOVED) & ~VALID if r else FLAG_OF_STATUS[s]
                         for s, r in zip(self.status, self.removed)], np.uint8)

    def valid(self):
        return int((self.key_status() == 0).sum())

    def remove(self, idx):
        """(result per candidate, distinct indices removed, those among them that had status 0)."""
        before = [NOT_IN_RANGE if i >= len(self) else (WAS_REMOVED if self.removed[i] else self.status[i]) for i in map(int, idx)]
        fresh = {int(i) for i, b in zip(idx, before) if b in (0, 1, 3)}
        for i in fresh:
            self.removed[i] = True
        return np.array(before, np.uint8), len(fresh), sum(self.status[i] == 0 for i in fresh)

    def lookup(self):
        return kc.model(self.rows, [r or s == 3 for s, r in zip(self.status, self.removed)])[0]

    def find(self, rows):
        d = self.lookup()
        return np.array([d.get(r, MISS) for r in rows], np.uint32)

    def add(self, rows, status, unique):
        idx = []
        for r, s in zip(rows, status):
            if unique and s == 3:
                idx.append(MISS)
                continue
            hit = self.lookup().get(r) if unique else None
            if hit is None:
                hit = len(self)
                self.rows.append(r); self.status.append(int(s)); self.removed.append(False)
            idx.append(hit)
        return np.array(idx, np.uint32)

    def compact(self):
        """(map, the model of the survivors)."""
        keep = [i for i in range(len(self)) if not self.removed[i]]
        m = np.full(len(self), GONE, np.uint32)
        m[keep] = np.arange(len(keep), dtype=np.uint32)
        return m, Model([self.rows[i] for i in keep], [self.status[i] for i in keep])


def triple(n: int):
    """The three indices one key is registered at: the first, a middle and the last key of the set."""
    return (0, n // 2, n - 1) if n >= 3 else ()


def shape(n: int):
    """(status per key, the indices that share one row): a malformed key at 1 and a key that is not `is_valid` at 3 where the
    set has room for them beside the triple."""
    status = [0] * n
    t = triple(n)
    if n >= 4 and 1 not in t:
        status[1] = 3
    if n >= 5 and 3 not in t:
        status[3] = 1
    return status, t


_host_sets = {}


def host_set(n: int, cols: int):
    """n keys of random canonical coordinates (distinct, but for the triple).  Returns (rows, status)."""
    if (n, cols) not in _host_sets:
        rng = np.random.default_rng(77 * n + cols)
        rows = [kc.rand_row(rng, cols) for _ in range(n)]
        status, t = shape(n)
        for i in t[1:]:
            rows[i] = rows[t[0]]
        _host_sets[(n, cols)] = (rows, status)
    return _host_sets[(n, cols)]


def patterns(n: int):
    """[(name, the idx column of one jjs_keyset_remove call)] for a set of n keys laid out by shape(n)."""
    out = [("first", [0]), ("last", [n - 1]), ("all_but_one", [i for i in range(n) if i != n // 3]), ("every_second", list(range(0, n, 2))),
           ("twice_and_out_of_range", [n - 1, n, 0, n - 1, 0xFFFFFFFF, 0])]
    if n >= 128:
        out.append(("one_wave", list(range(64, 128))))
    if n > 262:
        out.append(("across_a_block_edge", list(range(250, 263))))
    t = triple(n)
    if t:
        out += [("lowest_of_three", [t[0]]), ("middle_of_three", [t[1]]), ("highest_of_three", [t[2]]), ("two_of_three", [t[1], t[0]])]
    if n >= 4:
        out.append(("the_malformed_key", [1, 1]))
    return [(name, np.array(idx, np.uint32)) for name, idx in out]


# ---- the device tests: real keys with signatures ---------------------------------------------------------------------------------
_gpu_sets = {}


def gpu_set(scheme: str, n: int, seed: int = 900):
    """n keys laid out by shape(n): the 8 honest keys of keyset_add_cases.signed_batch spread over the set (key j at every index
    i with i % 8 == j, so every item's own key is there several times -- beyond the triple, duplicates everywhere: find must give
    the lowest survivor of each), the malformed and the status-1 key of shape(n).  Returns (rows, status, where: honest key j ->
    the indices that hold it)."""
    if (scheme, n) not in _gpu_sets:
        _, h = ac.signed_batch(scheme, 16385, 8, seed)
        cols = COLS[scheme]
        status, t = shape(n)
        # a few hundred distinct keys beside the honest ones, so that the lookup table is not eight chains
        filler = ac.chain_rows(cols, max(GPU_COUNTS)) if n > 8 else None
        rows = [h[i % 8] if i % 3 == 0 or n <= 8 else filler[i] for i in range(n)]
        for i in t[1:]:
            rows[i] = rows[t[0]]
        for i, s in enumerate(status):
            if s == 3:
                rows[i] = kc.o.le32(kc.o.Q) + rows[i][32:]
            elif s == 1:
                rows[i] = kc.IDENT + rows[i][64:]
        where = {j: [i for i in range(n) if rows[i] == h[j]] for j in range(8)}
        _gpu_sets[(scheme, n)] = (rows, status, where)
    return _gpu_sets[(scheme, n)]


def with_ff(rows, removed):
    """The key list jjs_keyset_remove's contract compares with: every removed key replaced by 0xFF bytes."""
    return [FF_ROW * (len(r) // 64) if gone else r for r, gone in zip(rows, removed)]


_items = {}


def items_over(scheme: str, rows, where, n: int, seed: int = 900, oracle: bool = False):
    """The first n items of the scheme's signed batch.  Item i names an index that holds its own key (where[i % 8], taken in
    turn); every fifth item index (7 * i) % len(rows) instead -- every index of a small set, a spread of a large one -- and every
    101st an index beyond the set.  Returns (key_idx, signature columns and messages, the statuses the C oracle gives with the
    named row inline (3 for a row that is not canonical or beyond the set) or None)."""
    from helpers import oracle_verify
    key = (scheme, tuple(rows), n, seed, oracle)
    if key in _items:
        return _items[key]
    b, _ = ac.signed_batch(scheme, 16385, 8, seed)
    b = {k: np.ascontiguousarray(v[:n]) for k, v in b.items()}
    idx = ((7 * np.arange(n)) % len(rows)).astype(np.uint32)
    for i in range(n):
        own = where.get(i % 8)
        if own and i % 5:
            idx[i] = own[(i // 8) % len(own)]
    beyond = np.arange(7, n, 101)
    idx[beyond] = len(rows)
    want = None
    if oracle:
        canon = [all(kc._canonical(p) for p in ac._pts(r)) for r in rows]
        stand_in = next(r for r, c in zip(rows, canon) if c)          # (the oracle is given points; what it says of these items is not kept)
        named = np.frombuffer(b"".join(rows[int(i)] if i < len(rows) and canon[int(i)] else stand_in for i in idx), np.uint8).reshape(n, -1)
        b2 = dict(b)
        for c, name in enumerate(ac.KEYCOLS[scheme]):
            b2[name] = np.ascontiguousarray(named[:, 64 * c:64 * c + 64])
        want = oracle_verify(scheme, b2, threads=16).copy().astype(np.uint8)
        want[beyond] = 3
        want[[k for k, i in enumerate(idx) if i < len(rows) and not canon[int(i)]]] = 3
    sig = [b["u"]] + [b[k] for k in ac.RCOLS[scheme]] + [b["m"]]
    _items[key] = (idx, sig, want)
    return _items[key]

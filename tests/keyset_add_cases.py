"""Adding keys to a live key set (csrc/keyset_add.h): the Python model every add is checked against -- a dict from a key's
canonical affine row to the lowest index it is registered at (JJS_KEYSET_ADD_UNIQUE), a list (JJS_KEYSET_ADD_APPEND) -- and the
sets and candidate lists shared by tests/test_keyset_add_host.py (CPU build) and tests/keyset_add_child.py (device).

The candidates of a scheme are drawn from 6 distinct new keys plus: a key already in the set; a key registered at two indices
(the lower must be returned); an affine coordinate >= q; a wire v >= q; an extended point with Z = 0; an off-curve affine
point (status 1, registered).  Every candidate is given as the bytes the call takes in its format; the model computes the
canonical row jjs_keyset_create would store for it on its own (normalisation, decoding), so it does not depend on how the
candidate was crafted."""
import numpy as np

import jjs_oracle as o
import keyset_lookup_cases as kc

MISS = 0xFFFFFFFF
COUNTS = (1, 255, 256, 257, 65537)          # the block edge (256 candidates) and the edge of the 256 x 256 two-level scan
COLS = {"single": 1, "double": 2, "vargen": 2}
WIDTH = {"affine": 64, "ext": 96, "wire": 32}
_row_cache, _status_cache = {}, {}


def _pts(row, w=64):
    return [row[p:p + w] for p in range(0, len(row), w)]


def canonical_row(enc: bytes, fmt: str):
    """The affine row(s) jjs_keyset_create stores for a candidate given as `enc` in `fmt`, or None for a malformed one: a
    coordinate >= q (extended: Z too), an encoding that does not decode.  An extended point with Z = 0 is stored as (0, 0)."""
    key = (fmt, enc)
    if key not in _row_cache:
        out = []
        for p in _pts(enc, WIDTH[fmt]):
            if fmt == "affine":
                out.append(p if kc._canonical(p) else None)
            elif fmt == "ext":
                U, V, Z = (int.from_bytes(p[k:k + 32], "little") for k in (0, 32, 64))
                if U >= o.Q or V >= o.Q or Z >= o.Q:
                    out.append(None)
                elif Z == 0:
                    out.append(bytes(64))
                else:
                    zi = o.fq_inv(Z)
                    out.append(o.le32(U * zi % o.Q) + o.le32(V * zi % o.Q))
            else:
                d = o.decompress(p)
                out.append(None if d is None else o.le32(d[0]) + o.le32(d[1]))
        _row_cache[key] = None if any(x is None for x in out) else b"".join(out)
    return _row_cache[key]


def row_status(row) -> int:
    """key_status of a canonical row (None: malformed): 0 when every point `is_valid`, else 1."""
    if row is None:
        return 3
    if row not in _status_cache:
        ok = all(o.point_is_valid((int.from_bytes(p[:32], "little"), int.from_bytes(p[32:], "little"))) for p in _pts(row))
        _status_cache[row] = 0 if ok else 1
    return _status_cache[row]


def unique_model(held, bad, rows):
    """held, bad: the set (its rows, its malformed flags); rows: the candidates' canonical rows (None: malformed).  Returns
    (idx per candidate, the rows the set gains in order, the candidates answered with an index that already existed)."""
    affine, _ = kc.model(held, bad)
    idx, new, seen, known = [], [], {}, 0
    for r in rows:
        if r is None:
            idx.append(MISS)
        elif r in affine:
            idx.append(affine[r]); known += 1
        else:
            if r not in seen:
                seen[r] = len(held) + len(new)
                new.append(r)
            idx.append(seen[r])
    return np.array(idx, np.uint32), new, known


def point(k: int) -> bytes:
    return kc.curve_point(k)


def key_rows(cols: int, first: int, count: int):
    """`count` distinct valid keys of `cols` points: multiples of the generator nobody else here uses."""
    return [b"".join(point(first + 97 * i + 13 * c) for c in range(cols)) for i in range(count)]


def base_set(scheme: str):
    """The set the candidates are offered to: six keys, the one at index 1 registered again at index 4, a malformed key at 3.
    Returns (held rows, malformed flags)."""
    cols = COLS[scheme]
    ks = key_rows(cols, 1000, 6)
    ks[4] = ks[1]
    ks[3] = o.le32(o.Q) + ks[3][32:]
    return ks, [0, 0, 0, 1, 0, 0]


def encode(row: bytes, fmt: str, z: int = 1) -> bytes:
    if fmt == "affine":
        return row
    if fmt == "ext":
        return b"".join(kc.to_ext(p, z) if kc._canonical(p) else p + o.le32(1) for p in _pts(row))
    return b"".join(kc.encoding(p) for p in _pts(row))


def pool(scheme: str, fmt: str):
    """The encodings the candidate lists draw from, as (name, bytes)."""
    cols = COLS[scheme]
    held, _ = base_set(scheme)
    new = key_rows(cols, 5000, 6)
    out = []
    for i, r in enumerate(new):
        out.append((f"new{i}", encode(r, fmt, 2 + i)))
        if fmt == "ext":                           # the same key at another Z: one canonical row
            out.append((f"new{i}z", encode(r, fmt, 1000003 + i)))
    out.append(("in_set", encode(held[0], fmt, 7)))
    out.append(("registered_twice", encode(held[1], fmt, 9)))
    out.append(("identity", encode(kc.IDENT + new[4][64:], fmt, 13)))       # decodes, on the curve, not `is_valid`: registered, status 1
    twin = kc.off_curve_twin(new[0][:64]) + new[0][64:]
    last = WIDTH[fmt] * (cols - 1)                 # the unusable point is the LAST of the key
    if fmt == "wire":
        out.append(("v_ge_q", encode(new[1], fmt)[:last] + kc.UNDECODABLE))
        out.append(("twin_encoding", encode(twin, fmt)))          # decodes to new0
    else:
        big = new[2][:64 * (cols - 1)] + o.le32(o.Q + 3) + new[2][64 * (cols - 1) + 32:]
        out.append(("coordinate_ge_q", encode(big, fmt)))
        out.append(("off_curve", encode(twin, fmt, 11)))
    if fmt == "ext":
        e = encode(new[3], fmt, 5)
        out.append(("z0", e[:last + 64] + o.le32(0)))
        out.append(("z_ge_q", e[:last + 64] + o.le32(o.Q)))
    return out


def candidates(scheme: str, fmt: str, n: int):
    """n candidates: the whole pool once in order (as far as n reaches), then draws from it.  Returns the encodings."""
    p = [e for _, e in pool(scheme, fmt)]
    rng = np.random.default_rng(n * 7 + len(fmt) + COLS[scheme])
    if n == 1:
        return [p[0]]
    # a duplicate AHEAD of the key's bulk: first occurrences are decided by position, not by count
    head = [p[-1], p[1], p[0]] + p
    draws = rng.integers(0, len(p), size=max(0, n - len(head)))
    return (head + [p[k] for k in draws])[:n]


SPREAD_KEYS, SPREAD_N = 300, 1300
_chain = {}


def chain_rows(cols: int, count: int):
    """`count` distinct valid keys of `cols` points by repeated addition of the generator (cheap: one addition per point)."""
    if (cols, count) not in _chain:
        p = o.mul(o.G, 900001)
        pts = []
        for _ in range(cols * count):
            p = o.add(p, o.G)
            pts.append(o.le32(p[0]) + o.le32(p[1]))
        _chain[(cols, count)] = [b"".join(pts[cols * i:cols * i + cols]) for i in range(count)]
    return _chain[(cols, count)]


def spread_candidates(scheme: str, fmt: str):
    """SPREAD_N candidates whose first occurrences lie in every wave of several blocks: SPREAD_KEYS distinct new keys (more than
    one block of NEW keys) and 1 000 draws from them and from the pool, in one random order -- duplicates ahead of and behind
    the first occurrences, which are at scattered ranks inside their blocks."""
    cols = COLS[scheme]
    rng = np.random.default_rng(4242 + len(fmt) + cols)
    base = [encode(r, fmt, 17 + i) for i, r in enumerate(chain_rows(cols, SPREAD_KEYS))]
    again = [encode(r, fmt, 40017 + i) for i, r in enumerate(chain_rows(cols, SPREAD_KEYS))]     # (ext: the same key at another Z)
    p = [e for _, e in pool(scheme, fmt)]
    src = again + p + p
    encs = base + [src[k] for k in rng.integers(0, len(src), SPREAD_N - SPREAD_KEYS)]
    return [encs[k] for k in rng.permutation(len(encs))]


def columns(encs, scheme: str, fmt: str):
    """The key columns jjs_keyset_add takes: (keys, keys2 | None)."""
    cols = COLS[scheme]
    a = np.frombuffer(b"".join(encs), np.uint8).reshape(len(encs), -1)
    if fmt == "wire":
        return np.ascontiguousarray(a), None
    w = WIDTH[fmt]
    c = [np.ascontiguousarray(a[:, w * i:w * i + w]) for i in range(cols)] + [None] * (2 - cols)
    return c[0], c[1]


def row_columns(rows, cols: int):
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 64 * cols)
    return [np.ascontiguousarray(a[:, 64 * i:64 * i + 64]) for i in range(cols)] + [None] * (2 - cols)


# ---- real keys with signatures for the device tests (tests/test_keyset_add_gpu.py, tests/keyset_add_child.py) ---------------------
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}
_batches = {}


def signed_batch(scheme: str, n: int, n_keys: int, seed: int):
    """helpers.make_batch, kept: item i is signed by honest key i % n_keys; some items are corrupt.  Returns (batch, the honest
    keys as rows)."""
    from helpers import make_batch
    key = (scheme, n, n_keys, seed)
    if key not in _batches:
        b = make_batch(scheme, n, seed=seed, n_keys=n_keys)
        h = make_batch(scheme, n_keys, seed=seed, n_keys=n_keys, mix=False)      # the same seed and key count: the same keys
        rows = [r.tobytes() for r in np.ascontiguousarray(np.concatenate([h[k] for k in KEYCOLS[scheme]], 1))]
        assert len(set(rows)) == n_keys
        _batches[key] = (b, rows)
    return _batches[key]


def append_keys(scheme: str, k1: int, seed: int = 900):
    """The key list of the APPEND test as affine rows: K1 = k1 honest keys, K2 = a malformed key (status 3), K3 = two honest
    keys, a key whose first point is the identity (status 1), an honest key and K1's first key again.  Returns (rows, the index
    of the honest key j or None, the index of the status-1 key, of the malformed key)."""
    _, h = signed_batch(scheme, 16385, 8, seed)
    mal = o.le32(o.Q) + h[7][32:]
    ident = kc.IDENT + h[6][64:]
    rows = h[:k1] + [mal] + [h[k1], h[k1 + 1], ident, h[k1 + 2], h[0]]
    where = {j: rows.index(h[j]) for j in range(8) if h[j] in rows}
    return rows, where, k1 + 3, k1


def encode_key(row: bytes, fmt: str, z: int) -> bytes:
    """`encode`, and for the wire format a first point that does not decode where the row's first point is not canonical."""
    if fmt == "wire" and not kc._canonical(row[:64]):
        return kc.UNDECODABLE + encode(row[64:], fmt) if len(row) > 64 else kc.UNDECODABLE
    return encode(row, fmt, z)


_items = {}


def items_over(scheme: str, rows, where, status1_at: int, malformed_at: int, n: int, seed: int = 900, oracle: bool = True):
    """The first n items of the scheme's signed batch with a key index each into `rows`: the item's own key where the list holds
    it, else another; some items name the status-1 key, the malformed key, an index beyond the list.  Returns (key_idx, the
    signature columns and messages (affine), the statuses the C oracle gives with the named key inline -- None without `oracle`)."""
    from helpers import oracle_verify
    key = (scheme, tuple(rows), n, seed, oracle)
    if key in _items:
        return _items[key]
    b, _ = signed_batch(scheme, 16385, 8, seed)
    b = {k: np.ascontiguousarray(v[:n]) for k, v in b.items()}
    idx = np.array([where.get(i % 8, i % len(rows)) for i in range(n)], np.uint32)
    idx[np.arange(5, n, 13)] = status1_at
    idx[np.arange(3, n, 17)] = malformed_at
    beyond = np.arange(7, n, 101)
    idx[beyond] = len(rows)
    named = np.frombuffer(b"".join(rows[min(int(i), len(rows) - 1)] for i in idx), np.uint8).reshape(n, -1)
    b2 = dict(b)
    for c, name in enumerate(KEYCOLS[scheme]):
        b2[name] = np.ascontiguousarray(named[:, 64 * c:64 * c + 64])
    want = None
    if oracle:
        want = oracle_verify(scheme, b2, threads=16).copy().astype(np.uint8)
        want[idx == malformed_at] = 3
        want[beyond] = 3
    sig = [b["u"]] + [b[k] for k in RCOLS[scheme]] + [b["m"]]
    _items[key] = (idx, sig, want)
    return _items[key]

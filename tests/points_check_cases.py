"""The case lists of `is_valid` alone (jjs_keys_check / jjs_signatures_check), shared by tests/test_points_check_host.py and
tests/test_points_check_gpu.py, with the answers of the oracle: oracle.point_is_valid, oracle.decompress and Python integers.

A point case is (input bytes in the format, status, affine output row); an item is one or two of them and, for a signature, a
scalar.  build(kind, scheme, fmt) gives the columns of the ABI call, the statuses, the tally and every output row.  Computed once
per process and never modified (the arrays are read-only)."""
from __future__ import annotations

import functools

import numpy as np

import jjs_oracle as o
from helpers import fe_bytes, pt_bytes, to_extended, to_pt, torsion_generator, wire_point_cases

SCHEMES = {"single": 0, "double": 1, "vargen": 2}
FORMATS = {"affine": 0, "ext": 1, "wire": 2}
ZERO64 = np.zeros(64, np.uint8)
TOP = (1 << 256) - 1
_valid = {}


def is_valid(p) -> bool:
    if p not in _valid:
        _valid[p] = o.point_is_valid(p)
    return _valid[p]


def affine_answer(u: int, v: int):
    """(status, output row) of the affine point (u, v) given as integers below 2^256."""
    if u >= o.Q or v >= o.Q:
        return 3, ZERO64
    return (0 if is_valid((u, v)) else 1), pt_bytes((u, v))


def ext_answer(row):
    U, V, Z = (int.from_bytes(bytes(row[i:i + 32]), "little") for i in (0, 32, 64))
    if U >= o.Q or V >= o.Q or Z >= o.Q:
        return 3, ZERO64
    if Z == 0:
        return 1, ZERO64
    zi = pow(Z, o.Q - 2, o.Q)
    p = (U * zi % o.Q, V * zi % o.Q)
    return (0 if is_valid(p) else 1), pt_bytes(p)


def wire_answer(enc: bytes):
    p = o.decompress(enc)
    if p is None:
        return 3, ZERO64
    return (0 if is_valid(p) else 1), pt_bytes(p)


def _raw_pt(u: int, v: int) -> np.ndarray:
    return np.frombuffer(u.to_bytes(32, "little") + v.to_bytes(32, "little"), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def valid_points():
    rng = np.random.default_rng(0x15A11D)
    return tuple(o.mul(o.G, int.from_bytes(rng.bytes(31), "little") + 1) for _ in range(16))


@functools.lru_cache(maxsize=None)
def affine_rows():
    """The affine point list: 16 valid, k T8, valid + k T8, off the curve, out of range."""
    rng = np.random.default_rng(0xAFF1)
    t8 = torsion_generator()
    rows = [pt_bytes(p) for p in valid_points()]
    rows += [pt_bytes(o.mul(t8, k) if k else o.IDENTITY) for k in range(8)]
    rows += [pt_bytes(o.add(valid_points()[k], o.mul(t8, k))) for k in range(1, 8)]
    for _ in range(4):
        rows.append(_raw_pt(int.from_bytes(rng.bytes(40), "little") % o.Q, int.from_bytes(rng.bytes(40), "little") % o.Q))
    for p in valid_points()[:4]:
        rows.append(_raw_pt(p[0], (p[1] + 1) % o.Q))
    for i, big in enumerate((o.Q, o.Q + 1, TOP)):
        p = valid_points()[i]
        rows.append(_raw_pt(big, p[1]))
        rows.append(_raw_pt(p[0], big))
        rows.append(_raw_pt(big, big))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def point_cases(fmt: str):
    """[(input row, status, output row)] of one point column in `fmt`."""
    rng = np.random.default_rng(0xC0FFEE)
    if fmt == "affine":
        return tuple((r, *affine_answer(*to_pt(r))) for r in affine_rows())
    if fmt == "ext":
        aff = np.stack(affine_rows())
        rows = list(to_extended(aff, rng, z_one_every=0)) + list(to_extended(aff, rng, z_one_every=1))
        one = fe_bytes(1)
        for r in affine_rows()[-9:]:                                    # the coordinates >= q as they are, with Z = 1 and a random Z
            rows.append(np.concatenate([r, one]))
            rows.append(np.concatenate([r, fe_bytes(int.from_bytes(rng.bytes(40), "little") % (o.Q - 1) + 1)]))
        p = valid_points()[5]
        z0 = fe_bytes(0)
        rows.append(np.concatenate([pt_bytes(p), z0]))                  # Z = 0, U and V arbitrary
        rows.append(np.concatenate([_raw_pt(7, 9), z0]))
        rows.append(np.concatenate([pt_bytes(o.IDENTITY), z0]))
        rows.append(np.zeros(96, np.uint8))                             # U = V = Z = 0
        for big in (o.Q, TOP):
            rows.append(np.concatenate([pt_bytes(p), np.frombuffer(big.to_bytes(32, "little"), np.uint8)]))
        for z in (1, 2, int.from_bytes(rng.bytes(40), "little") % (o.Q - 1) + 1):
            rows.append(np.concatenate([fe_bytes(0), fe_bytes(z), fe_bytes(z)]))     # the identity as (0 : Z : Z)
        return tuple((np.ascontiguousarray(r, np.uint8), *ext_answer(r)) for r in rows)
    assert fmt == "wire"
    return tuple((np.frombuffer(e, np.uint8).copy(), *wire_answer(e)) for e in wire_point_cases(rng, n_random=16))


def _first(cases, status):
    return next(c for c in cases if c[1] == status)


@functools.lru_cache(maxsize=None)
def build(kind: str, scheme: str, fmt: str):
    """kind 'keys' or 'signatures'.  Returns a dict: cols (the input columns of the ABI call, None where the format has none),
    status, tally, outs (keys: [A0, A1]; signatures: [u, R, R']; None where the scheme has no such output), n_valid_item (the
    index of an item with status 0, the padding of the GPU test)."""
    pts = point_cases(fmt)
    n_pts = (1 if scheme == "single" else 2) if kind == "keys" else (2 if scheme == "double" else 1)
    good = [c for c in pts if c[1] == 0]
    rng = np.random.default_rng(0x5CA1A5)
    items = []                                    # ([point cases], scalar or None)

    def scalar():
        return int.from_bytes(rng.bytes(40), "little") % o.R_ORDER if kind == "signatures" else None

    for i, c in enumerate(pts):                   # every point case, in the columns in turn beside a valid point
        if n_pts == 1:
            items.append(([c], scalar()))
        else:
            other = good[i % len(good)]
            items.append(([c, other] if i % 2 == 0 else [other, c], scalar()))
    if n_pts == 2:                                # one representative per class, every pair
        for a in (0, 1, 3):
            for b in (0, 1, 3):
                items.append(([_first(pts, a), _first(pts, b)], scalar()))
    if kind == "signatures":
        for j, u in enumerate((0, o.R_ORDER - 1, o.R_ORDER, TOP) * 3):           # three times: status 3 by the scalar alone, too
            items.append(([good[(j + k) % len(good)] for k in range(n_pts)], u))
        items.append(([_first(pts, 1)] * n_pts, o.R_ORDER))                   # a scalar out of range beside an invalid point: 3
    n = len(items)
    status = np.array([max([c[1] for c in cs] + [3 if (u is not None and u >= o.R_ORDER) else 0]) for cs, u in items], np.uint8)
    for k in (0, 1, 3):
        assert int((status == k).sum()) >= 8, (kind, scheme, fmt, k, int((status == k).sum()))
    assert not (status == 2).any()
    col = [np.stack([cs[k][0] for cs, _ in items]) for k in range(n_pts)]
    out = [np.stack([ZERO64 if status[i] == 3 else cs[k][2] for i, (cs, _) in enumerate(items)]) for k in range(n_pts)] + [None] * (2 - n_pts)
    if kind == "keys":
        cols = [np.concatenate(col, 1), None] if fmt == "wire" else [col[0], col[1] if n_pts == 2 else None]
        outs = out
    else:
        u = np.stack([np.frombuffer(x.to_bytes(32, "little"), np.uint8) for _, x in items])
        cols = [np.concatenate([u] + col, 1), None, None] if fmt == "wire" else [u, col[0], col[1] if n_pts == 2 else None]
        u_out = u.copy()
        u_out[status == 3] = 0
        outs = [u_out] + out
    r = {"cols": [None if c is None else np.ascontiguousarray(c) for c in cols], "status": status,
         "tally": np.array([int((status == k).sum()) for k in range(4)], np.uint64), "outs": outs, "n": n,
         "n_valid_item": int(np.where(status == 0)[0][0])}
    for a in r["cols"] + r["outs"] + [r["status"], r["tally"]]:
        if a is not None:
            a.setflags(write=False)
    return r


def padded(case, n: int, at_end: bool):
    """The case list as a call of n items: padded with copies of a valid item -- the cases in the last rows (at_end) or the
    first -- or, when it has more than n items, its last (first) n."""
    m = case["n"]
    if n <= m:
        idx = np.arange(m - n, m) if at_end else np.arange(n)
    else:
        pad = np.full(n - m, case["n_valid_item"])
        idx = np.concatenate([pad, np.arange(m)]) if at_end else np.concatenate([np.arange(m), pad])
    take = lambda a: None if a is None else np.ascontiguousarray(a[idx])  # noqa: E731
    st = case["status"][idx]
    return {"cols": [take(c) for c in case["cols"]], "status": st, "tally": np.array([int((st == k).sum()) for k in range(4)], np.uint64),
            "outs": [take(a) for a in case["outs"]], "n": n}


ALL = [(kind, scheme, fmt) for kind in ("keys", "signatures") for scheme in SCHEMES for fmt in FORMATS]

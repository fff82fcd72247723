"""Wire forms of the multisignature cases (jjs_multisig_*_wire*, jjs_msig_group_*_wire*), shared by the CPU build
(test_msig_wire_host.py) and the device (test_msig_wire_gpu.py).

A `WireCase` turns a `multisig_cases.Case` into wire columns: every point of PK, R and S becomes the 32 bytes of
`jjs_oracle.compress`.  Then points are planted.  UNDECODABLE encodings -- v = q, 32 x 0xFF, a v < q whose u^2 is not a square
(found by search from a seed), v = 1 with the sign bit, v = q - 1 with the sign bit (u = 0 with the sign bit set) -- and DECODABLE
edge encodings, which must pass through with no status of their own: v = 1 (the identity), v = q - 1 (order 2), v = 0 with both
signs (order 4), and a point with an odd and one with an even u.  The case keeps the DERIVED affine case beside the wire columns:
every decodable encoding the point `jjs_oracle.decompress` gives in Python integers, every undecodable one 64 bytes of 0xFF,
marked as a coordinate >= q the way `Case.bad_coord` marks one, so that `multisig_cases.expected` / `check` apply to the derived
case unchanged.  The contract is that a _wire call gives, byte for byte, what the affine call gives on `derived`.

Everything here is Python integers over the case's own bytes; nothing comes from the code under test."""
from __future__ import annotations

import numpy as np

import jjs_oracle as o
import multisig_cases as mc

POINT_COLS = ("PK", "R", "S")
UNDECODABLE = ("v=q", "0xFF", "non-residue", "v=1 signed", "v=q-1 signed")
DECODABLE = ("identity", "order 2", "order 4 +", "order 4 -", "odd u", "even u")
KINDS = UNDECODABLE + DECODABLE
SIGN = 1 << 255


def _search(seed: int, want_point: bool) -> int:
    """The first v >= seed below q whose u^2 = (v^2 - 1) / (1 + d v^2) is a non-zero square (want_point) or no square."""
    v = seed % o.Q
    while True:
        p = o.decompress(o.le32(v))
        if (p is not None and p[0] != 0) if want_point else (p is None and o.decompress(o.le32(v | SIGN)) is None):
            return v
        v += 1


def encoding(kind: str, seed: int = 0x5EED) -> bytes:
    """The 32 bytes of a planted kind."""
    if kind == "v=q":
        return o.le32(o.Q)
    if kind == "0xFF":
        return b"\xff" * 32
    if kind == "non-residue":
        return o.le32(_search(seed, False))
    if kind == "v=1 signed":
        return o.le32(1 | SIGN)
    if kind == "v=q-1 signed":
        return o.le32((o.Q - 1) | SIGN)
    if kind == "identity":
        return o.le32(1)
    if kind == "order 2":
        return o.le32(o.Q - 1)
    if kind == "order 4 +":
        return o.le32(0)
    if kind == "order 4 -":
        return o.le32(SIGN)
    v = _search(seed + 1000, True)
    return o.le32(v | SIGN) if kind == "odd u" else o.le32(v)        # the sign bit is the parity of u


def compress_column(aff: np.ndarray) -> np.ndarray:
    """(n, 64) canonical affine points -> (n, 32) with jjs_oracle.compress."""
    out = np.empty((len(aff), 32), np.uint8)
    for i, row in enumerate(aff):
        u, v = int.from_bytes(row[:32].tobytes(), "little"), int.from_bytes(row[32:].tobytes(), "little")
        assert u < o.Q and v < o.Q, "only canonical points have a wire form"
        out[i] = np.frombuffer(o.compress((u, v)), np.uint8)
    return out


def derive_row(row32: np.ndarray) -> np.ndarray:
    p = o.decompress(row32.tobytes())
    if p is None:
        return np.full(64, 0xFF, np.uint8)
    return np.frombuffer(o.le32(p[0]) + o.le32(p[1]), np.uint8)


def derive_column(wire: np.ndarray) -> np.ndarray:
    """The derived affine column of a wire one, from Python integers: decoded points, 0xFF rows."""
    return np.array([derive_row(r) for r in wire], np.uint8).reshape(len(wire), 64)


def undecodable(row32: np.ndarray) -> bool:
    return o.decompress(row32.tobytes()) is None


class WireCase:
    """wire: {"PK", "R", "S"} -> (N, 32) for the code under test; derived: the `multisig_cases.Case` the affine call takes."""

    def __init__(self, case: mc.Case, seed: int = 0x5EED):
        assert not any(kind == "coord" for _, kind, _, _ in case.marks), "build the wire form first, then plant"
        self.derived = mc.Case(case.clean, case.offsets, case.planned, case.dirty, case.marks)
        self.wire = {c: compress_column(case.dirty[c]) for c in POINT_COLS}
        self.seed = seed
        self.plants = []                       # (t, j, col, kind)

    @property
    def n(self):
        return self.derived.n

    @property
    def T(self):
        return self.derived.T

    def plant(self, t: int, j: int, col: str, kind: str) -> None:
        i = self.derived.row(t, j)
        assert not any((t, j, col) == p[:3] for p in self.plants), "one plant per point"
        enc = np.frombuffer(encoding(kind, self.seed), np.uint8)
        self.wire[col][i] = enc
        if kind in UNDECODABLE:
            assert undecodable(enc)
            self.derived.dirty[col][i] = 0xFF
            self.derived.marks.append((t, "coord", j, col))
        else:
            p = o.decompress(enc.tobytes())
            assert p is not None and o.is_on_curve(p)
            self.derived.set_point(t, j, col, p)               # the oracle sees it: no status of its own
        self.plants.append((t, j, col, kind))

    def args(self):
        """z, PK_w, R_w, S_w, m, offsets."""
        d = self.derived.dirty
        return [d["z"], self.wire["PK"], self.wire["R"], self.wire["S"], d["m"], self.derived.offsets.astype(np.uint32)]

    def check_derived(self) -> None:
        """The derived columns are the decodings of the wire ones (the case's own consistency, in Python integers)."""
        for c in POINT_COLS:
            assert (derive_column(self.wire[c]) == self.derived.dirty[c]).all(), c


def places(x: WireCase, boundary: int):
    """The first row of the call, a middle row, the last row, and both sides of the boundary between transcripts `boundary`
    and `boundary + 1`: five rows in five transcripts."""
    sizes = x.derived.sizes()
    first = min(t for t in range(x.T) if sizes[t])
    last = max(t for t in range(x.T) if sizes[t])
    mid = next(t for t in range(x.T // 4, x.T) if sizes[t] >= 3 and t not in (boundary, boundary + 1))
    out = [(first, 0), (mid, int(sizes[mid]) // 2), (last, int(sizes[last]) - 1), (boundary, int(sizes[boundary]) - 1), (boundary + 1, 0)]
    assert all(sizes[t] for t, _ in out) and len({t for t, _ in out}) == 5
    return out


def plant_everywhere(x: WireCase, boundary: int) -> None:
    """Every undecodable kind in every point column, one per (place, column) of the five places -- five kinds, three columns,
    kind k of column c at place (k + c) % 5, so that every place holds three kinds and every kind sits at three places; in
    transcript `boundary + 2` one undecodable R beside a good PK and a good S in its row; and every decodable edge kind in every
    column, three to a row (one per column), in the rows in the middle of six transcripts that hold nothing else."""
    sizes = x.derived.sizes()
    at = places(x, boundary)
    for c, col in enumerate(POINT_COLS):
        for k, kind in enumerate(UNDECODABLE):
            x.plant(*at[(k + c) % 5], col, kind)
    taken = {t for t, _ in at} | {boundary + 2}
    assert sizes[boundary + 2] and boundary + 2 not in {t for t, _ in at}
    x.plant(boundary + 2, int(sizes[boundary + 2]) // 2, "R", "non-residue")
    free = [t for t in range(x.T) if sizes[t] and t not in taken]
    assert len(free) >= len(DECODABLE)
    step = len(free) // len(DECODABLE)
    for k in range(len(DECODABLE)):
        t = free[k * step]
        for c, col in enumerate(POINT_COLS):
            x.plant(t, int(sizes[t]) // 2, col, DECODABLE[(k + c) % len(DECODABLE)])
    assert {(col, kind) for _, _, col, kind in x.plants} == {(col, kind) for col in POINT_COLS for kind in KINDS}


def sig_rows(u: np.ndarray, R_w: np.ndarray) -> np.ndarray:
    """(B, 32) u and (B, 32) compressed R -> (B, 64) = u || R, Signature::to_bytes."""
    return np.ascontiguousarray(np.concatenate([u, R_w], axis=1), dtype=np.uint8)

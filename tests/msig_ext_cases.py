"""Extended-coordinate forms of the multisignature cases (jjs_multisig_combine_ext_dev, jjs_msig_group_*_ext, the host forms),
shared by the CPU build (test_msig_ext_host.py) and the device (test_msig_ext_gpu.py).

An `ExtCase` turns a `multisig_cases.Case` into extended columns: every point (u, v) of PK, R and S becomes (u Z, v Z, Z) mod q
with a random non-zero Z per point (the first points of the call get the chosen Z = 1, q - 1, 2), then UNUSABLE points are
planted -- Z = 0, Z = q, Z = 2^256 - 1, U = q, V = q + 1 (include/jjs_gpu.h: a point is unusable when U, V or Z >= q or Z = 0).
It keeps the DERIVED affine case beside them: every usable point the canonical (U / Z, V / Z), every unusable one 64 bytes of
0xFF, marked as a coordinate >= q the way `Case.bad_coord` marks one, so that `multisig_cases.expected` / `check` apply to the
derived case unchanged.  The contract is that an _ext call gives, byte for byte, what the affine call gives on `derived`.

Everything here is Python integers over the case's own bytes; nothing comes from the code under test."""
from __future__ import annotations

import numpy as np

import jjs_oracle as o
import multisig_cases as mc

POINT_COLS = ("PK", "R", "S")
KINDS = ("Z=0", "Z=q", "Z=2^256-1", "U=q", "V=q+1")
CHOSEN_Z = (1, o.Q - 1, 2)


def _le(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8)


def to_ext_column(aff: np.ndarray, rng, chosen=()) -> np.ndarray:
    """(n, 64) canonical affine points -> (n, 96) U || V || Z with Z random in [1, q), `chosen` for the first rows."""
    n = len(aff)
    out = np.empty((n, 96), np.uint8)
    zb = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    zb[:, 31] &= 0x3F                              # < 2^254 < q
    zb[:, 0] |= 1                                  # non-zero
    for i in range(n):
        u, v = int.from_bytes(aff[i, :32].tobytes(), "little"), int.from_bytes(aff[i, 32:].tobytes(), "little")
        assert u < o.Q and v < o.Q, "only canonical points have an extended form"
        z = chosen[i] if i < len(chosen) else int.from_bytes(zb[i].tobytes(), "little")
        assert 0 < z < o.Q
        out[i, :32], out[i, 32:64], out[i, 64:] = _le(u * z % o.Q), _le(v * z % o.Q), _le(z)
    return out


def unusable(row96: np.ndarray) -> bool:
    U, V, Z = (int.from_bytes(row96[k:k + 32].tobytes(), "little") for k in (0, 32, 64))
    return U >= o.Q or V >= o.Q or Z >= o.Q or Z == 0


def derive_column(ext: np.ndarray) -> np.ndarray:
    """The derived affine column of an extended one, from Python integers: canonical quotients, 0xFF rows."""
    out = np.empty((len(ext), 64), np.uint8)
    for i, row in enumerate(ext):
        if unusable(row):
            out[i] = 0xFF
            continue
        U, V, Z = (int.from_bytes(row[k:k + 32].tobytes(), "little") for k in (0, 32, 64))
        zi = pow(Z, -1, o.Q)
        out[i, :32], out[i, 32:] = _le(U * zi % o.Q), _le(V * zi % o.Q)
    return out


def spoil(row96: np.ndarray, kind: str) -> None:
    """Makes the extended point unusable, in place."""
    at, value = {"Z=0": (64, 0), "Z=q": (64, o.Q), "Z=2^256-1": (64, mc.ALL_ONES), "U=q": (0, o.Q), "V=q+1": (32, o.Q + 1)}[kind]
    row96[at:at + 32] = _le(value)


class ExtCase:
    """ext: {"PK", "R", "S"} -> (N, 96) for the code under test; derived: the `multisig_cases.Case` the affine call takes."""

    def __init__(self, case: mc.Case, seed: int):
        assert not any(kind == "coord" for _, kind, _, _ in case.marks), "build the extended form first, then plant"
        rng = np.random.default_rng(seed)
        self.derived = mc.Case(case.clean, case.offsets, case.planned, case.dirty, case.marks)
        self.ext = {c: to_ext_column(case.dirty[c], rng, CHOSEN_Z if c == "R" else CHOSEN_Z[k:k + 1]) for k, c in enumerate(POINT_COLS)}
        self.plants = []                       # (t, j, col, kind)

    @property
    def n(self):
        return self.derived.n

    @property
    def T(self):
        return self.derived.T

    def plant(self, t: int, j: int, col: str, kind: str) -> None:
        i = self.derived.row(t, j)
        spoil(self.ext[col][i], kind)
        assert unusable(self.ext[col][i])
        self.derived.dirty[col][i] = 0xFF
        self.derived.marks.append((t, "coord", j, col))
        self.plants.append((t, j, col, kind))

    def args(self):
        """z, PK_ext, R_ext, S_ext, m, offsets."""
        d = self.derived.dirty
        return [d["z"], self.ext["PK"], self.ext["R"], self.ext["S"], d["m"], self.derived.offsets.astype(np.uint32)]

    def check_derived(self) -> None:
        """The derived columns are the quotients of the extended ones (the case's own consistency, in Python integers)."""
        for c in POINT_COLS:
            assert (derive_column(self.ext[c]) == self.derived.dirty[c]).all(), c


def tile_ext(x: ExtCase, reps: int) -> ExtCase:
    y = ExtCase.__new__(ExtCase)
    y.derived = mc.tile(x.derived, reps)
    y.ext = {c: np.tile(x.ext[c], (reps, 1)) for c in POINT_COLS}
    y.plants = [(t + r * x.T, j, col, kind) for r in range(reps) for t, j, col, kind in x.plants]
    return y


def plant_everywhere(x: ExtCase, boundary: int) -> None:
    """Every kind in every column, spread over four places: the first row of the call, the last row, and both sides of the
    boundary between transcripts `boundary` and `boundary + 1` (all four transcripts non-empty); and in transcript
    `boundary + 2` one unusable R beside a good PK and a good S in its row."""
    sizes = x.derived.sizes()
    last = max(t for t in range(x.T) if sizes[t])
    first = min(t for t in range(x.T) if sizes[t])
    places = [(first, 0), (last, int(sizes[last]) - 1), (boundary, int(sizes[boundary]) - 1), (boundary + 1, 0)]
    assert all(sizes[t] for t, _ in places) and len({t for t, _ in places}) == 4
    k = 0
    for col in POINT_COLS:
        for kind in KINDS:
            x.plant(*places[k % 4], col, kind)
            k += 1
    assert {(t, j) for t, j, _, _ in x.plants} == set(places)
    assert sizes[boundary + 2] and boundary + 2 not in {t for t, _ in places}
    x.plant(boundary + 2, int(sizes[boundary + 2]) // 2, "R", "Z=0")


def concat_ext(*xs) -> ExtCase:
    y = ExtCase.__new__(ExtCase)
    y.derived = mc.concat(*[x.derived for x in xs])
    y.ext = {c: np.concatenate([x.ext[c] for x in xs]) for c in POINT_COLS}
    y.plants, T = [], 0
    for x in xs:
        y.plants += [(t + T, j, col, kind) for t, j, col, kind in x.plants]
        T += x.T
    return y

"""Cases for the multisignature batch (jjs_multisig_combine_dev, csrc/multisig_core.h), shared by the CPU build
(test_multisig_host.py) and the device (test_multisig_gpu.py), and what both are compared with.

Inputs: transcripts signed with known secret keys, so that a transcript of n participants costs 3 n + 2 scalar multiplications
of the C oracle: d_i from the oracle's sponge, pk_agg = (sum d_i sk_i) G, a, RSa = (sum r_i + a sum s_i) G, c and
z_i = r_i + s_i a - c d_i sk_i (reference src/multisig.rs:213-257, 440-500).  This only PRODUCES inputs; whether they are valid
is the oracle's word (`expected` asserts that the oracle gives every share the status the builder planned).

Expected values: jjs_oracle_c.multisig_combine (the reference's algorithm), never the engine.  It defines all five outputs of
every transcript whose encodings are canonical.  A `Case` therefore keeps two sets of arrays: `clean` (every encoding
canonical) goes to the oracle, `dirty` (clean plus the out-of-range encodings of `marks`) goes to the code under test, and
`expected` derives the dirty transcripts' outputs from the clean ones by the rules of include/jjs_gpu.h:
  m >= q            every share 3, transcript 3, no signature; agg_pk does not depend on m: the clean transcript's
  z_j >= r          share j 3; z enters no hash and no other share's equation: the other shares and agg_pk as in the clean
                    transcript; no signature; transcript status = its first non-zero share
  coordinate >= q   share j 3, no signature, transcript status non-zero, and 3 when j is the transcript's first share.  The other
                    shares' statuses depend on arithmetic over an out-of-range value, which nothing defines: NOT compared (nor is
                    agg_pk when the coordinate is one of PK).  `check` counts these shares and caps them below 2 % of the call.
"""
from __future__ import annotations

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc
from helpers import pt_bytes, torsion_generator

MASK250 = (1 << 250) - 1
COOP_MAX_ITEMS = 8192          # csrc/engine_state.h MSIG_COOP_MAX_ITEMS: a hash pass with at most this many items runs on 8 lanes each
TABLE_PARTICIPANTS = 256       # csrc/jjs_sponge_tags_long.inc JJS_MSIG_MAX_PARTICIPANTS: the last row of the generated tag table
COLS = ("z", "PK", "R", "S", "m")
ALL_ONES = (1 << 256) - 1


def lane_modes(n: int, T: int):
    """Lanes per item of passes 1, 2 and 4 as the launch rule of jjs_gpu.hip gives them."""
    one = 8 if n <= COOP_MAX_ITEMS else 1
    two = 8 if T <= COOP_MAX_ITEMS else 1
    return one, two, two


def _fe(xs) -> np.ndarray:
    if not len(xs):
        return np.zeros((0, 32), np.uint8)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), np.uint8).reshape(-1, 32).copy()


def _ints(a) -> list:
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def _scalars(rng, n) -> list:
    b = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    b[:, 31] &= 0x07                       # < 2^251 < r
    b[:, 0] |= 1
    return _ints(b)


class Case:
    """One call: `dirty` arrays for the code under test, `clean` arrays for the oracle, offsets, the planned share statuses
    (0, 4, or -1 where the builder makes no claim) and the out-of-range encodings: marks = [(t, kind, j, col)] with kind
    "z" | "m" | "coord" and col "PK" | "R" | "S" for a coordinate."""

    def __init__(self, clean, offsets, planned, dirty=None, marks=()):
        self.clean = {k: np.array(clean[k], np.uint8, order="C") for k in COLS}          # copies: a slice does not alias its source
        self.dirty = {k: np.array((dirty or clean)[k], np.uint8, order="C") for k in COLS}
        self.offsets = np.array(offsets, np.int64)
        self.planned = np.array(planned, np.int16)
        self.marks = list(marks)

    @property
    def n(self):
        return int(self.offsets[-1])

    @property
    def T(self):
        return len(self.offsets) - 1

    def sizes(self):
        return np.diff(self.offsets)

    def args(self):
        """What a `run(z, PK, R, S, m, offsets)` takes."""
        return [self.dirty[k] for k in COLS] + [self.offsets.astype(np.uint32)]

    def row(self, t, j):
        assert 0 <= j < self.offsets[t + 1] - self.offsets[t], (t, j)
        return int(self.offsets[t]) + j

    # ---- changes that keep every encoding canonical (the oracle sees them) ----
    def set_z(self, t, j, value, planned=4):
        i = self.row(t, j)
        self.clean["z"][i] = self.dirty["z"][i] = _fe([value])[0]
        self.planned[i] = planned

    def corrupt(self, t, j):
        i = self.row(t, j)
        self.set_z(t, j, (_ints(self.clean["z"][i:i + 1])[0] + 1) % o.R_ORDER)

    def set_m(self, t, value):
        self.clean["m"][t] = self.dirty["m"][t] = _fe([value])[0]
        self.planned[self.offsets[t]:self.offsets[t + 1]] = -1

    def set_point(self, t, j, col, point):
        """An on-curve point in place of a participant's PK, R or S: every hash of the transcript changes."""
        i = self.row(t, j)
        self.clean[col][i] = self.dirty[col][i] = pt_bytes(point)
        self.planned[self.offsets[t]:self.offsets[t + 1]] = -1

    # ---- out-of-range encodings (the oracle does not see them) ----
    def bad_z(self, t, j, value):
        assert value >= o.R_ORDER
        self.dirty["z"][self.row(t, j)] = _fe([value])[0]
        self.marks.append((t, "z", j, None))

    def bad_m(self, t, value):
        assert value >= o.Q
        self.dirty["m"][t] = _fe([value])[0]
        self.marks.append((t, "m", 0, None))

    def bad_coord(self, t, j, col, half, value):
        assert value >= o.Q and col in ("PK", "R", "S") and half in (0, 1)
        self.dirty[col][self.row(t, j), 32 * half:32 * half + 32] = _fe([value])[0]
        self.marks.append((t, "coord", j, col))

    # ---- assembling calls ----
    def slice(self, t0, t1):
        lo, hi = int(self.offsets[t0]), int(self.offsets[t1])
        pick = lambda d: {k: (d[k][t0:t1] if k == "m" else d[k][lo:hi]) for k in COLS}  # noqa: E731
        marks = [(t - t0, kind, j, col) for t, kind, j, col in self.marks if t0 <= t < t1]
        return Case(pick(self.clean), self.offsets[t0:t1 + 1] - lo, self.planned[lo:hi], pick(self.dirty), marks)


def concat(*cases) -> Case:
    clean = {k: np.concatenate([c.clean[k] for c in cases]) for k in COLS}
    dirty = {k: np.concatenate([c.dirty[k] for c in cases]) for k in COLS}
    offs, marks, n, T = [np.zeros(1, np.int64)], [], 0, 0
    for c in cases:
        offs.append(c.offsets[1:] + n)
        marks += [(t + T, kind, j, col) for t, kind, j, col in c.marks]
        n += c.n; T += c.T
    return Case(clean, np.concatenate(offs), np.concatenate([c.planned for c in cases]), dirty, marks)


def tile(case: Case, reps: int) -> Case:
    """`reps` copies of a call, one behind the other."""
    rows = lambda d: {k: np.tile(d[k], (reps, 1)) for k in COLS}  # noqa: E731
    offs = np.concatenate([np.zeros(1, np.int64)] + [case.offsets[1:] + r * case.n for r in range(reps)])
    marks = [(t + r * case.T, kind, j, col) for r in range(reps) for t, kind, j, col in case.marks]
    return Case(rows(case.clean), offs, np.tile(case.planned, reps), rows(case.dirty), marks)


def valid_transcripts(sizes, seed, zero=(), threads=0) -> Case:
    """Transcripts of the given participant counts (0: an empty transcript) in which every share is valid.
    zero = [(t, j, "sk" | "r" | "s")]: that secret scalar is 0, so that PK_j, R_j or S_j is the identity and the share still valid."""
    sizes = [int(x) for x in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, T = int(offs[-1]), len(sizes)
    rng = np.random.default_rng(seed)
    sk, r, s = (_scalars(rng, N) for _ in range(3))
    for t, j, which in zero:
        assert j < sizes[t]
        {"sk": sk, "r": r, "s": s}[which][int(offs[t]) + j] = 0
    m = rng.integers(0, 256, (T, 32), dtype=np.uint8)
    m[:, 31] &= 0x3F                       # < 2^254 < q
    G = np.tile(pt_bytes(o.G), (max(N, T, 1), 1))
    PK, R, S = (oc.scalar_mul(G[:N], _fe(v), threads) for v in (sk, r, s))
    groups = {}
    for t, n in enumerate(sizes):
        if n:
            groups.setdefault(n, []).append(t)
    groups = {n: (np.array(ts), offs[np.array(ts)][:, None] + np.arange(n)[None, :]) for n, ts in groups.items()}
    d = [0] * N
    for n, (ts, idx) in groups.items():                       # d_i = H(pk_i, pk_lo .. pk_hi)
        pk = PK[idx]
        pre = np.empty((len(ts), n, 2 + 2 * n, 32), np.uint8)
        pre[:, :, 0] = pk[:, :, :32]; pre[:, :, 1] = pk[:, :, 32:]
        pre[:, :, 2::2] = pk[:, None, :, :32]; pre[:, :, 3::2] = pk[:, None, :, 32:]
        for i, v in zip(idx.reshape(-1), _ints(oc.poseidon_any(pre.reshape(-1, 2 + 2 * n, 32), threads))):
            d[int(i)] = v & MASK250
    span = lambda v, t: v[int(offs[t]):int(offs[t + 1])]  # noqa: E731
    AGG = oc.scalar_mul(G[:T], _fe([sum(x * k for x, k in zip(span(d, t), span(sk, t))) % o.R_ORDER for t in range(T)]), threads)
    a = [0] * T
    for n, (ts, idx) in groups.items():                       # a = H(pk_agg, m, R_lo, S_lo, ...)
        pre = np.empty((len(ts), 3 + 4 * n, 32), np.uint8)
        pre[:, 0] = AGG[ts, :32]; pre[:, 1] = AGG[ts, 32:]; pre[:, 2] = m[ts]
        pre[:, 3::4] = R[idx][:, :, :32]; pre[:, 4::4] = R[idx][:, :, 32:]
        pre[:, 5::4] = S[idx][:, :, :32]; pre[:, 6::4] = S[idx][:, :, 32:]
        for t, v in zip(ts, _ints(oc.poseidon_any(pre, threads))):
            a[int(t)] = v & MASK250
    RSA = oc.scalar_mul(G[:T], _fe([(sum(span(r, t)) + a[t] * sum(span(s, t))) % o.R_ORDER for t in range(T)]), threads)
    c5 = np.stack([RSA[:, :32], RSA[:, 32:], AGG[:, :32], AGG[:, 32:], m], 1) if T else np.zeros((0, 5, 32), np.uint8)
    c = [v & MASK250 for v in _ints(oc.poseidon(c5, threads))]
    z = []
    for t in range(T):
        z += [(ri + si * a[t] - c[t] * di * ki) % o.R_ORDER for ri, si, di, ki in zip(span(r, t), span(s, t), span(d, t), span(sk, t))]
    return Case({"z": _fe(z), "PK": PK, "R": R, "S": S, "m": m}, offs, np.zeros(N, np.int16))


def ragged_sizes(rng, total: int, top: int = 8) -> list:
    """Participant counts in 1 .. top, ones and twos among them, that sum to `total`."""
    assert total >= 3
    sizes, total = [2, 1], total - 3
    while total > 0:
        n = min(int(rng.integers(1, top + 1)), total)
        sizes.append(n); total -= n
    return sizes


def filler(total: int, seed: int, top: int = 8, threads: int = 0, every: int = 7) -> Case:
    """`total` shares in ragged valid transcripts; every `every`-th transcript has one share off by one (status 4)."""
    rng = np.random.default_rng(seed)
    case = valid_transcripts(ragged_sizes(rng, total, top), seed + 1, threads=threads)
    for t in range(3, case.T, every):
        case.corrupt(t, int(rng.integers(0, case.sizes()[t])))
    return case


def straddles(case: Case, k: int) -> bool:
    """Some transcript has shares on both sides of a multiple of k."""
    lo, hi = case.offsets[:-1], case.offsets[1:]
    return bool(((hi - 1) // k > lo // k).any())


# ---- the special transcripts -------------------------------------------------------------------------------------------------
POSITIONS = ("first", "middle", "last")


def _pos(n, where):
    return {"first": 0, "middle": n // 2, "last": n - 1}[where]


def malformed_case(seed: int = 500, threads: int = 0):
    """Every range test of msig_share_item at the first, a middle and the last participant of a transcript of its own:
    z = r, 2^256 - 1 (malformed), r - 1, 0 (valid encodings of wrong shares); each of the six coordinates = q and one = 2^256 - 1;
    m = q, 2^256 - 1 (malformed) and q - 1 (canonical).  Returns the case and [(t, what, j)] for messages."""
    zvals = [("z=r", o.R_ORDER, True), ("z=2^256-1", ALL_ONES, True), ("z=r-1", o.R_ORDER - 1, False), ("z=0", 0, False)]
    coords = [(f"{col}.{'uv'[half]}=q", col, half, o.Q) for col in ("PK", "R", "S") for half in (0, 1)] + [("R.u=2^256-1", "R", 0, ALL_ONES)]
    sizes = [3 + (k + i) % 3 for k in range(len(zvals)) for i in range(3)] + [3] * (3 * len(coords)) + [2, 3, 1]
    case = valid_transcripts(sizes, seed, threads=threads)
    names, t = [], 0
    for what, value, bad in zvals:
        for where in POSITIONS:
            j = _pos(sizes[t], where)
            case.bad_z(t, j, value) if bad else case.set_z(t, j, value)
            names.append((t, what, j)); t += 1
    for what, col, half, value in coords:
        for where in POSITIONS:
            j = _pos(3, where)
            case.bad_coord(t, j, col, half, value)
            names.append((t, what, j)); t += 1
    case.bad_m(t, o.Q); names.append((t, "m=q", 0)); t += 1
    case.bad_m(t, ALL_ONES); names.append((t, "m=2^256-1", 0)); t += 1
    case.set_m(t, o.Q - 1); names.append((t, "m=q-1", 0)); t += 1
    assert t == case.T
    return case, names


def first_failure_case(seed: int = 600, threads: int = 0):
    """Two different failures in one transcript, in both orders, and transcripts whose only bad share is the last one.
    Returns the case and the transcript statuses written out by hand: the status of the FIRST failing share."""
    case = valid_transcripts([5, 5, 4, 4, 6, 6, 2], seed, threads=threads)
    want = []
    case.corrupt(0, 1); case.bad_z(0, 3, o.R_ORDER); want.append(4)            # 4 before 3
    case.bad_z(1, 1, ALL_ONES); case.corrupt(1, 3); want.append(3)             # 3 before 4
    case.corrupt(2, 3); want.append(4)                                         # only the last share, invalid
    case.bad_z(3, 3, o.R_ORDER + 1); want.append(3)                            # only the last share, malformed
    case.corrupt(4, 0); case.bad_z(4, 5, o.R_ORDER); want.append(4)            # first and last
    case.bad_z(5, 0, o.R_ORDER); case.corrupt(5, 5); want.append(3)
    want.append(0)                                                             # a good transcript beside them
    return case, want


def small_order_points():
    t8 = torsion_generator()
    assert o.mul(t8, 4) == o.ORDER2 and o.mul(t8, 8) == o.IDENTITY
    return [("identity", o.IDENTITY), ("order 2", o.ORDER2), ("order 8", t8)]


def small_order_case(seed: int = 700, threads: int = 0):
    """Identity, the point of order 2 and a point of order 8 as PK, R and S in turn (on the curve, so the result is defined;
    they go through build_point_table, table_mul and to_affine_words), in transcripts of 2 to 4 participants; then transcripts
    that stay VALID with identity points in them (a secret scalar of 0), one of which consists of identities only, so that
    agg_pk and RSa are the identity as well.  Returns the case and the first transcript of the valid part."""
    points = small_order_points()
    sizes = [2 + (k % 3) for k in range(9)]
    zero = [(9, 1, "sk"), (10, 0, "r"), (11, 2, "s"), (12, 0, "sk"), (12, 0, "r"), (12, 0, "s"), (13, 0, "sk"), (13, 1, "sk")]
    case = valid_transcripts(sizes + [3, 2, 4, 1, 2], seed, zero=zero, threads=threads)
    t = 0
    for col in ("PK", "R", "S"):
        for k, (_, pt) in enumerate(points):
            case.set_point(t, (t + k) % sizes[t], col, pt)
            t += 1
    ident = pt_bytes(o.IDENTITY)
    assert (case.clean["PK"][case.row(9, 1)] == ident).all() and (case.clean["S"][case.row(11, 2)] == ident).all()
    return case, 9


def specials(seed: int = 0, threads: int = 0) -> Case:
    return concat(malformed_case(500 + seed, threads)[0], first_failure_case(600 + seed, threads)[0], small_order_case(700 + seed, threads)[0])


def empty_layout_sizes(rng, T: int, shares: int, top: int = 6) -> list:
    """T transcripts of which many are empty, with `shares` participants in all: empty transcripts at the first two and the last
    two indices, in runs in between, and single ones between non-empty neighbours."""
    full = ragged_sizes(rng, shares, top)
    assert len(full) + 8 <= T
    sizes = [0] * T
    inner = np.sort(rng.choice(np.arange(2, T - 2), len(full), replace=False))
    for t, n in zip(inner, full):
        sizes[int(t)] = n
    return sizes


# ---- expected values and the comparison -----------------------------------------------------------------------------
class Expected:
    pass


def expected(case: Case, threads: int = 0) -> Expected:
    e = Expected()
    c = case.clean
    st, ts, agg, su, sr = oc.multisig_combine(c["z"], c["PK"], c["R"], c["S"], c["m"], case.offsets.astype(np.uint32), threads=threads)
    st, ts, agg, su, sr = st.copy(), ts.copy(), agg.copy(), su.copy(), sr.copy()
    known = case.planned >= 0
    assert (st[known] == case.planned[known]).all(), "the oracle disagrees with the builder's plan"
    e.cmp_share = np.ones(case.n, bool)
    e.cmp_agg = np.ones(case.T, bool)
    e.ts_exact = np.ones(case.T, bool)
    e.coord_transcripts = set()
    by_t = {}
    for t, kind, j, col in case.marks:
        by_t.setdefault(t, []).append((kind, j, col))
    for t, ms in by_t.items():
        lo, hi = int(case.offsets[t]), int(case.offsets[t + 1])
        kinds = {kind for kind, _, _ in ms}
        su[t] = 0; sr[t] = 0
        if "coord" in kinds:
            e.coord_transcripts.add(t)
            e.cmp_share[lo:hi] = False
            if any(col == "PK" for kind, _, col in ms if kind == "coord"):
                e.cmp_agg[t] = False
        for kind, j, _ in ms:
            if kind == "m":
                st[lo:hi] = 3; e.cmp_share[lo:hi] = True
            else:
                st[lo + j] = 3; e.cmp_share[lo + j] = True
        if "coord" in kinds:
            first_is_bad = bool(e.cmp_share[lo] and st[lo] == 3)
            ts[t] = 3 if first_is_bad else 255          # 255: any non-zero status
            e.ts_exact[t] = first_is_bad
        else:
            nz = st[lo:hi][st[lo:hi] != 0]
            ts[t] = nz[0]
    e.st, e.ts, e.agg, e.su, e.sr = st, ts, agg, su, sr
    e.uncompared = int((~e.cmp_share).sum())
    return e


def tile_expected(e: Expected, reps: int, T: int) -> Expected:
    x = Expected()
    for k in ("st", "ts", "cmp_share", "cmp_agg", "ts_exact"):
        setattr(x, k, np.tile(getattr(e, k), reps))
    for k in ("agg", "su", "sr"):
        setattr(x, k, np.tile(getattr(e, k), (reps, 1)))
    x.coord_transcripts = {t + r * T for r in range(reps) for t in e.coord_transcripts}
    x.uncompared = e.uncompared * reps
    return x


def check(case: Case, e: Expected, got, label: str = "") -> int:
    """Every output of a run against `e`; `got` in the order of Engine.multisig_combine: (share_status, agg_pk, sig_u, sig_R,
    transcript_status or None).  Returns the number of shares left uncompared, after asserting the cap on it."""
    st, agg, su, sr, ts = got
    assert st.shape == (case.n,) and agg.shape == (case.T, 64) and su.shape == (case.T, 32) and sr.shape == (case.T, 64), label
    tr_of = np.repeat(np.arange(case.T), case.sizes())
    bad = np.nonzero(e.cmp_share & (st != e.st))[0]
    assert not len(bad), (label, "share", bad[:8].tolist(), tr_of[bad[:8]].tolist(), st[bad[:8]].tolist(), e.st[bad[:8]].tolist())
    for name, g, w, mask in (("agg_pk", agg, e.agg, e.cmp_agg), ("sig_u", su, e.su, None), ("sig_R", sr, e.sr, None)):
        diff = (g != w).any(1)
        if mask is not None:
            diff &= mask
        assert not diff.any(), (label, name, np.nonzero(diff)[0][:8].tolist())
    if ts is not None:
        assert ts.shape == (case.T,), label
        diff = e.ts_exact & (ts != e.ts)
        assert not diff.any(), (label, "transcript_status", np.nonzero(diff)[0][:8].tolist(), ts[diff][:8].tolist(), e.ts[diff][:8].tolist())
        assert (ts[~e.ts_exact] != 0).all(), (label, "a transcript with a malformed share has status 0")
    # the one exclusion: shares beside a coordinate >= q.  Under 2 % of the call, and only in the transcripts built for it
    assert e.uncompared == int((~e.cmp_share).sum())
    assert e.uncompared * 50 < max(case.n, 1), (label, e.uncompared, case.n)
    assert set(tr_of[~e.cmp_share].tolist()) <= e.coord_transcripts, label
    assert e.coord_transcripts == {t for t, kind, _, _ in case.marks if kind == "coord"}, label
    return e.uncompared


def python_oracle_outputs(case: Case, t: int):
    """What the Python oracle (oracle/jjs_oracle.py) gives for transcript t of the clean arrays: (share statuses, transcript
    status, agg_pk, sig_u, sig_R) as bytes, by the definitions of include/jjs_gpu.h."""
    from helpers import to_int, to_pt
    lo, hi = int(case.offsets[t]), int(case.offsets[t + 1])
    c = case.clean
    zs = [to_int(x) for x in c["z"][lo:hi]]
    pks, Rs, Ss = ([to_pt(x) for x in c[k][lo:hi]] for k in ("PK", "R", "S"))
    msg = to_int(c["m"][t])
    ds, agg, a, rsa, ch = o.multisig_transcript(pks, Rs, Ss, msg)
    st = [0 if o.add(o.mul(o.G, z), o.mul(pk, ch * d % o.R_ORDER)) == o.add(Rp, o.mul(Sp, a)) else 4
          for z, pk, d, Rp, Sp in zip(zs, pks, ds, Rs, Ss)]
    first = next((x for x in st if x), 0)
    ok = first == 0
    return (st, first, pt_bytes(agg).tobytes(), o.le32(sum(zs) % o.R_ORDER) if ok else bytes(32),
            pt_bytes(rsa).tobytes() if ok else bytes(64))


# ---- calls that both builds run -------------------------------------------------------------------------------------------
def mixed_call(shares: int, seed: int, T: int = 0, threads: int = 0, top: int = 8):
    """The special transcripts in the middle of ragged filler, `shares` participants in all.  With T, the call has T transcripts,
    the surplus being empty ones (empty_layout_sizes).  Returns the case and where each special section starts."""
    mal, names = malformed_case(500 + seed, threads)
    ff, ff_want = first_failure_case(600 + seed, threads)
    so, so_valid = small_order_case(700 + seed, threads)
    n_special, T_special = mal.n + ff.n + so.n, mal.T + ff.T + so.T
    rng = np.random.default_rng(seed)
    if T:
        fill = valid_transcripts(empty_layout_sizes(rng, T - T_special, shares - n_special, top), seed + 1, threads=threads)
        for t in np.nonzero(fill.sizes())[0][3::7]:
            fill.corrupt(int(t), int(rng.integers(0, fill.sizes()[t])))
    else:
        fill = filler(shares - n_special, seed, top, threads)
    cut = fill.T // 2
    case = concat(fill.slice(0, cut), mal, ff, so, fill.slice(cut, fill.T))
    assert case.n == shares and (not T or case.T == T)
    sections = {"malformed": (cut, names), "first_failure": (cut + mal.T, ff_want), "small_order": (cut + mal.T + ff.T, so_valid)}
    return case, sections


def check_sections(case: Case, sections, got, label: str = ""):
    """What the special transcripts must give, written out without the oracle: the range tests, the first-failure rule,
    status 5 and cleared outputs for exactly the empty transcripts."""
    st, agg, su, sr, ts = got
    t0, names = sections["malformed"]
    for t, what, j in names:
        lo, hi = int(case.offsets[t0 + t]), int(case.offsets[t0 + t + 1])
        if what in ("m=q", "m=2^256-1"):
            assert st[lo:hi].tolist() == [3] * (hi - lo) and ts[t0 + t] == 3, (label, what)
        elif what == "m=q-1":
            assert 3 not in st[lo:hi].tolist() and ts[t0 + t] != 3, (label, what)
        elif what in ("z=r-1", "z=0"):
            assert st[lo + j] == 4 and ts[t0 + t] == 4, (label, what, j)
        else:
            assert st[lo + j] == 3 and ts[t0 + t] != 0, (label, what, j)
            assert ts[t0 + t] == 3 or j > 0, (label, what, j)
        if what != "m=q-1":
            assert not su[t0 + t].any() and not sr[t0 + t].any(), (label, what, j)
    t0, want = sections["first_failure"]
    assert ts[t0:t0 + len(want)].tolist() == want, label
    for k, w in enumerate(want):
        assert agg[t0 + k].any(), (label, k)
        assert bool(su[t0 + k].any()) == bool(sr[t0 + k].any()) == (w == 0), (label, k)
    empty = case.sizes() == 0
    assert ((ts == 5) == empty).all(), label
    assert not agg[empty].any() and not su[empty].any() and not sr[empty].any(), label


def state_calls(threads: int = 0) -> dict:
    """The calls of the scratch-reuse sequence (test_multisig_gpu.py, multisig_state_child.py).  "small" fits the scratch a first
    call allocates (4096 shares, 1024 transcripts); "grow" exceeds both; in "long_at_3" transcript 3 is beyond the tag table and
    transcript 5 is short, in "long_at_5" it is the other way round, so that a row of long_tags written by one call belongs to
    a short transcript in the next."""
    small, grow = filler(1501, 60, top=6, threads=threads), filler(5001, 61, top=4, threads=threads)
    assert small.n < 4096 and small.T < 1024 and grow.n > 4096 and grow.T > 1024
    at3 = valid_transcripts([2, 1, 3, 300, 4, 2, 5, 1], 62, threads=threads)
    at5 = valid_transcripts([2, 1, 3, 2, 4, 257, 5, 1], 63, threads=threads)
    at3.corrupt(3, 299); at3.corrupt(5, 0); at5.corrupt(5, 128); at5.corrupt(6, 4)
    return {"small": small, "grow": grow, "long_at_3": at3, "long_at_5": at5}


STATE_ORDER = ("small", "grow", "small", "long_at_3", "long_at_5", "long_at_3")
OUTPUTS = ("share_status", "agg_pk", "sig_u", "sig_R", "transcript_status")

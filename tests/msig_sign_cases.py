"""Cases for the signer's multisignature calls (jjs_multisig_round1_dev, jjs_multisig_sign*, csrc/msig_sign.h), shared by the CPU
build (test_msig_sign_host.py) and the device (test_msig_sign_gpu.py), and the Python model both are compared with.

A `SCase` is the transcripts of one call with the secrets of every participant row: PK, R, S (N, 64) -- or (N, 96) = U || V || Z in
the extended format -- m (B, 32), the offsets, and sk, r, s (N, 32).  `build` only PRODUCES inputs (the points are the C
oracle's scalar multiples of G); a test then plants what it is about straight into the arrays.  `call(rows)` gives the signing
columns of a call: signer_row (None: the whole-transcript generator) and the secrets of those rows.

Expected values (`model`): the reference's sign_round_2 written out in plain Python over the case's own bytes --
  * the structural checks of src/multisig.rs:218-246 (the key occurs exactly once; r G = R_i and s G = S_i; no R and no S
    twice in the transcript) with the precedence of include/jjs_gpu.h: 3 (a signing row beyond the call, a secret scalar >= r,
    any coordinate of the transcript >= q, m >= q) before 5 before 7;
  * the share: oracle.multisig_sign_share (oracle/jjs_oracle.py, pinned by the reference's KAT bytes) for a transcript of up to
    8 participants; for a longer one oracle.multisig_transcript once and z = r + s a - c d_i sk from its values, which is that
    function's last line (multisig_sign_share recomputes the transcript per share) -- `model` asserts both agree on the short ones.
An extended column is first turned into its derived affine column by msig_ext_cases.derive_column (Python integers; an unusable
point is 64 bytes of 0xFF, hence a coordinate >= q).  Nothing here comes from the code under test.

The transcript of 257 participants costs the Python oracle 257 hashes of 516 inputs, most of a minute; its model values are
recorded in tests/golden/msig_sign_257.npz by tests/golden/make_msig_sign_fixture.py (which runs `model`), keyed by a digest of
the inputs, so that the tests that use them stay quick."""
from __future__ import annotations

import hashlib
import os

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc
import msig_ext_cases as xc
import multisig_cases as mc
from helpers import pt_bytes, to_int, to_pt

NO_ROW = 0xFFFFFFFF
FIXTURE_257 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msig_sign_257.npz")


class SCase:
    def __init__(self, PK, R, S, m, offsets, sk, r, s, fmt="affine"):
        w = 96 if fmt == "ext" else 64
        self.fmt = fmt
        self.PK, self.R, self.S = (np.array(x, np.uint8, order="C").reshape(-1, w) for x in (PK, R, S))
        self.m, self.sk, self.r, self.s = (np.array(x, np.uint8, order="C").reshape(-1, 32) for x in (m, sk, r, s))
        self.offsets = np.array(offsets, np.int64)
        assert len(self.PK) == len(self.R) == len(self.S) == len(self.sk) == len(self.r) == len(self.s) == self.n and len(self.m) == self.B

    @property
    def n(self):
        return int(self.offsets[-1])

    @property
    def B(self):
        return len(self.offsets) - 1

    def offs32(self):
        return self.offsets.astype(np.uint32)

    def copy(self):
        return SCase(self.PK, self.R, self.S, self.m, self.offsets, self.sk, self.r, self.s, self.fmt)

    def row(self, t, j):
        assert 0 <= j < self.offsets[t + 1] - self.offsets[t], (t, j)
        return int(self.offsets[t]) + j

    def rows_of(self, t):
        return list(range(int(self.offsets[t]), int(self.offsets[t + 1])))

    def call(self, rows=None):
        """(signer_row, sk, r, s) of a call that signs `rows` (global rows, any order; None: every row, signer_row NULL)."""
        if rows is None:
            return None, self.sk.copy(), self.r.copy(), self.s.copy()
        rows = np.asarray(rows, np.int64)
        return rows.astype(np.uint32), self.sk[rows].copy(), self.r[rows].copy(), self.s[rows].copy()

    def affine(self):
        """The affine columns the passes work on: the case's own, or the derived ones of an extended case."""
        if self.fmt == "ext":
            return tuple(xc.derive_column(x) for x in (self.PK, self.R, self.S))
        return self.PK, self.R, self.S

    def to_ext(self, seed):
        """The same transcripts in the extended format with random Z != 1 (the first rows Z = 1, q - 1, 2)."""
        assert self.fmt == "affine"
        rng = np.random.default_rng(seed)
        PK, R, S = (xc.to_ext_column(x, rng, xc.CHOSEN_Z if k == 1 else ()) for k, x in enumerate((self.PK, self.R, self.S)))
        return SCase(PK, R, S, self.m, self.offsets, self.sk, self.r, self.s, "ext")

    def digest(self):
        h = hashlib.sha256()
        for x in (self.PK, self.R, self.S, self.m, self.offs32(), self.sk, self.r, self.s):
            h.update(np.ascontiguousarray(x).tobytes())
        return h.hexdigest()


def build(sizes, seed, threads=0) -> SCase:
    """Transcripts of the given participant counts (0: an empty transcript) with random secrets below 2^251."""
    sizes = [int(x) for x in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, B = int(offs[-1]), len(sizes)
    rng = np.random.default_rng(seed)
    sk, r, s = (mc._fe(mc._scalars(rng, N)) for _ in range(3))
    m = rng.integers(0, 256, (B, 32), dtype=np.uint8)
    m[:, 31] &= 0x3F                       # < 2^254 < q
    G = np.tile(pt_bytes(o.G), (max(N, 1), 1))[:N]
    PK, R, S = (oc.scalar_mul(G, v, threads) for v in (sk, r, s))
    return SCase(PK, R, S, m, offs, sk, r, s)


def kat_case(kat) -> SCase:
    """reference_kat.json["multisig_kat"] as one transcript of 3 participants (the points are the Python oracle's multiples)."""
    sks, rs, ss = kat["secret_keys"], kat["r_scalars"], kat["s_scalars"]
    pts = lambda v: np.stack([pt_bytes(o.mul(o.G, x)) for x in v])  # noqa: E731
    return SCase(pts(sks), pts(rs), pts(ss), mc._fe([kat["message"]]), [0, 3], mc._fe(sks), mc._fe(rs), mc._fe(ss))


# ---- the model -------------------------------------------------------------------------------------------------------------
def _big(row, mod):
    return any(to_int(row[k:k + 32]) >= mod for k in range(0, len(row), 32))


def model(c: SCase, signer_row, sk, r, s, recorded=None):
    """(z (k, 32), sign_status (k,)) of the call.  recorded: {transcript: (N_t, 32) shares of its rows} for transcripts whose
    model values come from a fixture this function wrote earlier."""
    PK, R, S = c.affine()
    N, B = c.n, c.B
    bad_enc, dup, repeats, tr_of = [False] * B, [False] * B, [False] * N, [0] * N
    for t in range(B):
        rows = c.rows_of(t)
        bad_enc[t] = bool(rows) and _big(c.m[t], o.Q)
        for i in rows:
            tr_of[i] = t
            bad_enc[t] = bad_enc[t] or _big(PK[i], o.Q) or _big(R[i], o.Q) or _big(S[i], o.Q)
            for k in rows:
                if k != i:
                    dup[t] = dup[t] or R[i].tobytes() == R[k].tobytes() or S[i].tobytes() == S[k].tobytes()
                    repeats[i] = repeats[i] or PK[i].tobytes() == PK[k].tobytes()
    k_sign = len(sk)
    rows = list(range(N)) if signer_row is None else [int(x) for x in signer_row]
    assert len(rows) == k_sign == len(r) == len(s)
    z, st = np.zeros((k_sign, 32), np.uint8), np.zeros(k_sign, np.uint8)
    transcripts = {}
    for j, i in enumerate(rows):
        if i >= N:
            st[j] = 3
            continue
        t = tr_of[i]
        x, rr, ss = to_int(sk[j]), to_int(r[j]), to_int(s[j])
        if x >= o.R_ORDER or rr >= o.R_ORDER or ss >= o.R_ORDER or bad_enc[t]:
            st[j] = 3
            continue
        if o.mul(o.G, x) != to_pt(PK[i]) or repeats[i] or o.mul(o.G, rr) != to_pt(R[i]) or o.mul(o.G, ss) != to_pt(S[i]):
            st[j] = 5
            continue
        if dup[t]:
            st[j] = 7
            continue
        lo, hi = int(c.offsets[t]), int(c.offsets[t + 1])
        if recorded is not None and t in recorded:
            z[j] = recorded[t][i - lo]
            continue
        pks, Rs, Ss = ([to_pt(v) for v in col[lo:hi]] for col in (PK, R, S))
        msg = to_int(c.m[t])
        if t not in transcripts:
            transcripts[t] = o.multisig_transcript(pks, Rs, Ss, msg)
        ds, _, a, _, ch = transcripts[t]
        share = (rr + ss * a - ch * ds[i - lo] * x) % o.R_ORDER
        if hi - lo <= 8:
            assert share == o.multisig_sign_share(x, rr, ss, pks, Rs, Ss, msg)
        z[j] = np.frombuffer(o.le32(share), np.uint8)
    return z, st


def check(got, want, label=""):
    (z, st), (wz, wst) = got, want
    assert st.tolist() == wst.tolist(), (label, "sign_status", st.tolist()[:64], wst.tolist()[:64])
    bad = np.nonzero((z != wz).any(1))[0]
    assert not len(bad), (label, "z", bad[:8].tolist())
    assert not z[st != 0].any(), (label, "a share behind a status other than 0")


# ---- the calls both builds run -----------------------------------------------------------------------------------------------
RAGGED_SIZES = (1, 2, 0, 3, 8)


def ragged(seed=1400, threads=0) -> SCase:
    """Transcripts of 1, 2, 3 and 8 participants with an empty transcript between them."""
    return build(RAGGED_SIZES, seed, threads)


def long_case(threads=0) -> SCase:
    """One transcript of 257 participants: one past the generated tag table."""
    assert mc.TABLE_PARTICIPANTS == 256
    return build([257], 1457, threads)


def recorded_257(c: SCase):
    """The fixture's shares of long_case(), after checking that they were recorded for exactly these inputs."""
    f = np.load(FIXTURE_257)
    assert str(f["digest"]) == c.digest(), "tests/golden/msig_sign_257.npz was recorded for other inputs: run make_msig_sign_fixture.py"
    return {0: f["z"]}


def point(k: int) -> np.ndarray:
    return pt_bytes(o.mul(o.G, k))


BASE_SIZES = (3, 4, 2)
TARGET = 1          # the transcript a rule case plants in; transcripts 0 and 2 must come out as in the clean call


class Rule:
    """One case of a rule: the call (case, signing rows and secrets) and what transcript TARGET's signing rows must give,
    written out by hand (`want`: the statuses of the signing rows of TARGET, in signing order)."""

    def __init__(self, name, case, rows, want, edit=None):
        self.name, self.case, self.want = name, case, want
        self.signer_row, self.sk, self.r, self.s = case.call(rows)
        if edit:
            edit(self)


def rule_cases(seed=1500, threads=0):
    """One case per rule of the share pass, each on a copy of one base call of transcripts of 3, 4 and 2 participants; every case
    signs every row (signer_row given), so signing row j is row j unless the case says otherwise."""
    base = build(BASE_SIZES, seed, threads)
    N = base.n
    every = list(range(N))
    lo = base.row(TARGET, 0)
    fe = lambda x: mc._fe([x])[0]  # noqa: E731
    out = []

    def add(name, want, plant=None, edit=None, fmt="affine"):
        c = base.copy()
        if fmt == "ext":
            c = c.to_ext(seed + 9)
        if plant:
            plant(c)
        out.append(Rule(name, c, every, want, edit))

    def set_signer(j, value):
        def edit(rule):
            rule.signer_row[j] = value
        return edit

    def set_secret(which, j, value):
        def edit(rule):
            getattr(rule, which)[j] = fe(value)
        return edit

    add("signer_row = N", [0, 3, 0, 0], edit=set_signer(lo + 1, N))
    add("signer_row = 0xFFFFFFFF", [0, 0, 0, 3], edit=set_signer(lo + 3, NO_ROW))
    for k, which in enumerate(("sk", "r", "s")):
        want = [0] * 4
        want[k] = 3
        add(which + " = r_order", want, edit=set_secret(which, lo + k, o.R_ORDER))

    def m_is_q(c):
        c.m[TARGET] = fe(o.Q)
    add("m = q", [3] * 4, m_is_q)

    def coord_is_q(c):
        c.S[lo + 2, 32:] = fe(o.Q)
    add("a coordinate = q in another row", [3] * 4, coord_is_q)

    def z_is_0(c):
        xc.spoil(c.R[lo + 3], "Z=0")
    add("an extended point with Z = 0", [3] * 4, z_is_0, fmt="ext")
    add("wrong sk", [0, 0, 5, 0], edit=set_secret("sk", lo + 2, 12345))
    add("the right sk at the wrong row", [0, 5, 0, 0], edit=set_signer(lo + 1, lo + 2))

    def key_twice(c):
        c.PK[lo + 3] = c.PK[lo]
    add("the signer's key at another row as well", [5, 0, 0, 5], key_twice)

    def other_R(c):
        c.R[lo + 1] = point(777)
    add("R[i] does not match", [0, 5, 0, 0], other_R)

    def other_S(c):
        c.S[lo] = point(778)
    add("S[i] does not match", [5, 0, 0, 0], other_S)

    def dup_of(col, secret):
        def plant(c):
            getattr(c, col)[lo + 3] = getattr(c, col)[lo + 1]
            getattr(c, secret)[lo + 3] = getattr(c, secret)[lo + 1]      # the nonce really is used twice: only rule 4 can object
        return plant
    add("R duplicated between two participants", [7] * 4, dup_of("R", "r"))
    add("S duplicated between two participants", [7] * 4, dup_of("S", "s"))
    add("a duplicate together with a wrong key", [5, 7, 7, 7], dup_of("R", "r"), edit=set_secret("sk", lo, 54321))

    def dup_and_bad(c):
        dup_of("S", "s")(c)
        c.PK[lo, :32] = fe(o.Q)
    add("a duplicate together with a bad encoding", [3] * 4, dup_and_bad)
    return base, out


def check_rule(rule: Rule, base_z, got, label=""):
    """What the hand-written expectation says: the statuses of TARGET's signing rows, z zero behind every status other than 0,
    and the other transcripts of the call exactly as the clean call gives them (base_z: the model's shares of the base call)."""
    z, st = got
    c = rule.case
    lo, hi = int(c.offsets[TARGET]), int(c.offsets[TARGET + 1])
    assert st[lo:hi].tolist() == rule.want, (label, rule.name, st[lo:hi].tolist())
    assert not z[st != 0].any(), (label, rule.name)
    others = [j for j in range(len(st)) if not lo <= j < hi]
    assert not st[others].any() and (z[others] == base_z[others]).all(), (label, rule.name, "the other transcripts")


def across_transcripts(seed=1600, threads=0) -> SCase:
    """Two different transcripts that share an R (and its secret): not a duplicate."""
    c = build([2, 3], seed, threads)
    c.R[c.row(1, 1)] = c.R[c.row(0, 0)]
    c.r[c.row(1, 1)] = c.r[c.row(0, 0)]
    return c


def combine_args(c: SCase, z):
    """z, PK, R, S, m, offsets: what the combine calls take for the case's transcripts and these shares."""
    return [np.ascontiguousarray(z), c.PK, c.R, c.S, c.m, c.offs32()]


def sum_mod_r(z) -> np.ndarray:
    return np.frombuffer(o.le32(sum(mc._ints(z)) % o.R_ORDER), np.uint8)

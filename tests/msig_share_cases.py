"""Cases for verify_share on its own (jjs_multisig_verify_share*, jjs_msig_group_verify_share*, jjs_multisig_verify_share_keyset*;
csrc/msig_share.h), shared by the CPU build (test_msig_share_host.py) and the device (test_msig_share_gpu.py).

A `ShareCase` is a `multisig_cases.Case` (built with multisig_cases.valid_transcripts, msig_group_cases.group_transcripts /
with_point / torsion_key_case or msig_keyset_cases.pool_transcripts) plus Q queries (transcript, slot, z).

Expected values never come from the code under test:
  status   of a query the rules 3 and 5 of include/jjs_gpu.h decide: written out from those rules (`plan`);
           of every other query (t, j, z): jjs_oracle_c.multisig_combine's share_status[j] on transcript t with z at row j --
           one oracle call for all of them, query q being transcript q of that call;
  sig_R    jjs_oracle.multisig_transcript's rsa for transcripts of up to 8 participants, for longer ones the C oracle's sig_R
           on the transcript with its signers' own shares, which must be valid; zero where rule 3 or 5 holds for the transcript.
Out-of-range encodings: an affine call gets the coordinates >= q the case's marks plant; an extended or wire call gets, at the
same rows, what poison mode turns into 0xFF rows (Z = 0, U = q; an encoding that does not decode, v = q).  m >= q is the same
in every format.
"""
from __future__ import annotations

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc
import msig_ext_cases as xc
import msig_group_cases as gcs
import msig_keyset_cases as kcs
import msig_wire_cases as wc
import multisig_cases as mc
from helpers import to_int, to_pt, pt_bytes

NO_INDEX = 0xFFFFFFFF
FORMATS = ("affine", "ext", "wire")
FORMAT_IDS = {"affine": 0, "ext": 1, "wire": 2}
PY_ORACLE_MAX = 8
EXT_SPOIL = ("Z=0", "U=q")
WIRE_SPOIL = ("non-residue", "v=q")


class ShareCase:
    """route "inline" | "group" | "keyset".  group: case is the tiled inline form of a group of group_n participants.  keyset:
    key_idx names the key of every row, refused = the transcripts that name an unusable one."""

    def __init__(self, route, case: mc.Case, key_idx=None, refused=(), group_pk=None, keys=None):
        self.route, self.case = route, case
        self.key_idx = None if key_idx is None else np.array(key_idx, np.uint32)
        self.refused = set(refused)
        self.group_pk, self.keys = group_pk, keys
        assert not any(kind == "z" for _, kind, _, _ in case.marks), "z comes with the queries"
        self.qt, self.qs, self.qz, self.what = [], [], [], []

    @property
    def T(self):
        return self.case.T

    @property
    def Q(self):
        return len(self.qt)

    def bad_transcripts(self):
        return {t for t, kind, _, _ in self.case.marks if kind in ("m", "coord")} | self.refused

    def ask(self, t, j, z=None, what=""):
        """One query; z None: the share the signer of (t, j) made."""
        if z is None:
            z = to_int(self.case.clean["z"][self.case.row(t, j)])
        self.qt.append(t); self.qs.append(j); self.qz.append(int(z)); self.what.append(what or f"({t}, {j})")

    def ask_all(self, skip=()):
        for t in range(self.T):
            if t not in skip:
                for j in range(int(self.case.sizes()[t])):
                    self.ask(t, j)

    def ask_edges(self, t3, t_rev, t_last):
        """The issue's list on top of ask_all: slot 0 of t3 three times (valid, corrupted, z >= r); two queries of t_rev in
        reverse order; slot == n and 2^32 - 1 of t_last and of every empty transcript; transcript == B and 2^32 - 1."""
        z0 = to_int(self.case.clean["z"][self.case.row(t3, 0)])
        self.ask(t3, 0, z0, "again"); self.ask(t3, 0, (z0 + 1) % o.R_ORDER, "corrupted"); self.ask(t3, 0, o.R_ORDER, "z = r")
        self.ask(t3, 0, mc.ALL_ONES, "z = 2^256 - 1")
        n = int(self.case.sizes()[t_rev])
        self.ask(t_rev, n - 1, None, "reverse order"); self.ask(t_rev, 0, None, "reverse order")
        self.ask(t_last, int(self.case.sizes()[t_last]), 5, "slot == n"); self.ask(t_last, NO_INDEX, 5, "slot 2^32 - 1")
        for t in np.nonzero(self.case.sizes() == 0)[0]:
            self.ask(int(t), 0, 5, "empty transcript")
        for t in self.bad_transcripts():
            self.ask(t, NO_INDEX, 5, "malformed transcript, slot 2^32 - 1")
        self.ask(self.T, 0, 5, "transcript == B"); self.ask(NO_INDEX, 0, 5, "transcript 2^32 - 1")

    def shuffle(self, seed):
        p = np.random.default_rng(seed).permutation(self.Q)
        for name in ("qt", "qs", "qz", "what"):
            setattr(self, name, [getattr(self, name)[i] for i in p])

    def queries(self):
        return np.array(self.qt, np.uint32), np.array(self.qs, np.uint32), mc._fe(self.qz)

    # ---- the columns of a call -----------------------------------------------------------------------------------------
    def columns(self, fmt, seed=5):
        """{"PK", "R", "S"} in format fmt for the code under test (PK: the inline column), and m."""
        c = self.case
        if fmt == "affine":
            return {k: c.dirty[k] for k in mc.COLS[1:4]}, c.dirty["m"]
        rng = np.random.default_rng(seed)
        if fmt == "ext":
            cols = {k: xc.to_ext_column(c.clean[k], rng) for k in mc.COLS[1:4]}
        else:
            cols = {k: wc.compress_column(c.clean[k]) for k in mc.COLS[1:4]}
        for k, (t, kind, j, col) in enumerate(m for m in c.marks if m[1] == "coord"):
            if fmt == "ext":
                xc.spoil(cols[col][c.row(t, j)], EXT_SPOIL[k % 2])
            else:
                cols[col][c.row(t, j)] = np.frombuffer(wc.encoding(WIRE_SPOIL[k % 2]), np.uint8)
        return cols, c.dirty["m"]

    def group_keys(self, fmt, seed=6):
        if fmt == "ext":
            return xc.to_ext_column(self.group_pk, np.random.default_rng(seed))
        return wc.compress_column(self.group_pk) if fmt == "wire" else self.group_pk


# ---- expected values ---------------------------------------------------------------------------------------------------------
def plan(sc: ShareCase):
    """Per query: the status rules 3 and 5 give it, or -1 where the equation decides."""
    bad, sizes, out = sc.bad_transcripts(), sc.case.sizes(), []
    for t, j, z in zip(sc.qt, sc.qs, sc.qz):
        if t >= sc.T or z >= o.R_ORDER or t in bad:
            out.append(3)
        elif j >= sizes[t]:
            out.append(5)
        else:
            out.append(-1)
    return np.array(out, np.int16)


def expected_status(sc: ShareCase, threads: int = 0) -> np.ndarray:
    want = plan(sc)
    open_q = np.nonzero(want < 0)[0]
    if not len(open_q):
        return want.astype(np.uint8)
    c, parts, rows, offs = sc.case, {k: [] for k in mc.COLS}, [], [0]
    for q in open_q:
        t, j = sc.qt[q], sc.qs[q]
        lo, hi = int(c.offsets[t]), int(c.offsets[t + 1])
        z = c.clean["z"][lo:hi].copy()
        z[j] = mc._fe([sc.qz[q]])[0]
        parts["z"].append(z)
        for k in ("PK", "R", "S"):
            parts[k].append(c.clean[k][lo:hi])
        parts["m"].append(c.clean["m"][t:t + 1])
        rows.append(offs[-1] + j)
        offs.append(offs[-1] + hi - lo)
    st = oc.multisig_combine(*[np.concatenate(parts[k]) for k in mc.COLS], np.array(offs, np.uint32), threads=threads)[0]
    want[open_q] = st[rows]
    assert set(want[open_q].tolist()) <= {0, 4}
    return want.astype(np.uint8)


def expected_R(sc: ShareCase, threads: int = 0) -> np.ndarray:
    c, bad = sc.case, sc.bad_transcripts()
    out = np.zeros((sc.T, 64), np.uint8)
    big = [t for t in range(sc.T) if c.sizes()[t] > PY_ORACLE_MAX and t not in bad]
    if big:
        _, ts, _, _, sr = oc.multisig_combine(*[c.clean[k] for k in mc.COLS], c.offsets.astype(np.uint32), threads=threads)
        for t in big:
            assert ts[t] == 0, "a long transcript's sig_R comes from the C oracle on valid shares"
            out[t] = sr[t]
    for t in range(sc.T):
        lo, hi = int(c.offsets[t]), int(c.offsets[t + 1])
        if t in bad or hi == lo or hi - lo > PY_ORACLE_MAX:
            continue
        pks, Rs, Ss = ([to_pt(x) for x in c.clean[k][lo:hi]] for k in ("PK", "R", "S"))
        out[t] = pt_bytes(o.multisig_transcript(pks, Rs, Ss, to_int(c.clean["m"][t]))[3])
    return out


def python_oracle_status(sc: ShareCase, q: int) -> int:
    """jjs_oracle.multisig_verify_share on query q (a query the equation decides)."""
    c, t, j = sc.case, sc.qt[q], sc.qs[q]
    lo, hi = int(c.offsets[t]), int(c.offsets[t + 1])
    pks, Rs, Ss = ([to_pt(x) for x in c.clean[k][lo:hi]] for k in ("PK", "R", "S"))
    return 0 if o.multisig_verify_share(sc.qz[q], j, pks, Rs, Ss, to_int(c.clean["m"][t])) else 4


def check(sc: ShareCase, want_st, want_R, got_st, got_R, label=""):
    got_st = np.asarray(got_st)
    assert got_st.shape == (sc.Q,), (label, got_st.shape)
    diff = np.nonzero(got_st != want_st)[0]
    assert not len(diff), (label, [(sc.what[i], sc.qt[i], sc.qs[i], int(got_st[i]), int(want_st[i])) for i in diff[:8]])
    if got_R is not None:
        got_R = np.asarray(got_R)
        assert got_R.shape == (sc.T, 64), (label, got_R.shape)
        diff = np.nonzero((got_R != want_R).any(1))[0]
        assert not len(diff), (label, "sig_R", diff[:8].tolist())


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _group_as_inline(gc: gcs.GroupCase) -> mc.Case:
    return gc.case


def small_order_groups(seed=40):
    """Groups of three whose key 1 is the identity, the order-2 point, an order-8 point (the shares stay as signed: the oracle
    decides), a group with secret key 0 and the same key twice, and torsion_key_case: a key with an order-8 part under which
    the reference ACCEPTS (R carries the matching part) -- c d_j reduced, and the sum identity outside the subgroup."""
    out = []
    for k, (name, pt) in enumerate(mc.small_order_points()):
        out.append((name, gcs.with_point(gcs.group_transcripts(3, 2, seed + k), 1, pt)))
    out.append(("sk 0, same key twice", gcs.group_transcripts(3, 2, seed + 5, zero_sk=(1,), same_sk=((2, 0),))))
    out.append(("torsion key", gcs.torsion_key_case()))
    return out


def inline_case(seed=20) -> ShareCase:
    """Ragged transcripts of 1, 2, 3, none, 8 participants; one nobody asks about; an R coordinate, m and a PK coordinate out of
    range, each between good neighbours; then the small-order and repeated-key transcripts in their inline form."""
    base = mc.valid_transcripts([1, 2, 3, 0, 8, 2, 3, 2, 3, 2, 3, 2], seed, zero=[(4, 2, "sk")])
    base.bad_coord(6, 1, "R", 0, o.Q)
    base.bad_m(8, o.Q)
    base.bad_coord(10, 2, "PK", 1, mc.ALL_ONES)
    case = mc.concat(base, *[gc.case for _, gc in small_order_groups(seed + 20)])
    sc = ShareCase("inline", case)
    sc.ask_all(skip=(5,))
    sc.ask_edges(t3=2, t_rev=4, t_last=11)
    sc.shuffle(seed)
    return sc


def group_cases(seed=60) -> list:
    """One ShareCase per group: a group of 4 over 5 transcripts with an S coordinate and an m out of range and a transcript
    without a query; a group of one; the small-order groups."""
    out = []
    gc = gcs.group_transcripts(4, 5, seed)
    gc.case.bad_coord(1, 3, "S", 1, o.Q)
    gc.case.bad_m(3, mc.ALL_ONES)
    sc = ShareCase("group", gc.case, group_pk=gc.PK)
    sc.ask_all(skip=(2,)); sc.ask_edges(t3=0, t_rev=4, t_last=4); sc.shuffle(seed)
    out.append(("group of 4", sc))
    gc = gcs.group_transcripts(1, 3, seed + 1)
    sc = ShareCase("group", gc.case, group_pk=gc.PK)
    sc.ask_all(); sc.ask_edges(t3=1, t_rev=2, t_last=0)
    out.append(("group of 1", sc))
    for name, gc in small_order_groups(seed + 20):
        sc = ShareCase("group", gc.case, group_pk=gc.PK)
        sc.ask_all(); sc.ask_edges(t3=0, t_rev=1, t_last=1)
        out.append((name, sc))
    return out


def keyset_case(seed=910) -> ShareCase:
    """msig_keyset_cases.host_mix without its z marks: ragged committees from the set's valid keys, the same key twice, an empty
    transcript, one refused transcript per cause, an R coordinate out of range."""
    keys, sk = kcs.key_set()
    kc, where = kcs.host_mix(keys, sk, seed, coord=True)
    c = kc.case
    c.marks = [m for m in c.marks if m[1] != "z"]
    c.dirty["z"] = c.clean["z"].copy()
    sc = ShareCase("keyset", c, key_idx=kc.key_idx, refused=kc.refused, keys=keys)
    sc.ask_all(skip=(where["good 2"],))
    sc.ask_edges(t3=where["good 3"], t_rev=where["good 8"], t_last=where["same key twice"])
    sc.shuffle(seed)
    return sc


def as_route(sc: ShareCase, route: str) -> ShareCase:
    """The same transcripts and queries for another route: a group case as an inline call on the tiled keys, a key-set case as
    an inline call on the gathered keys (its refused transcripts are ordinary ones there)."""
    assert route == "inline"
    x = ShareCase("inline", sc.case)
    x.qt, x.qs, x.qz, x.what = list(sc.qt), list(sc.qs), list(sc.qz), list(sc.what)
    return x

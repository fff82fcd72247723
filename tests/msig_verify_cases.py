"""Cases for the verifier's multisignature calls (jjs_multisig_aggregate_pk*, jjs_multisig_verify*, csrc/msig_verify.h), shared by
the CPU build (test_msig_verify_host.py) and the device (test_msig_verify_gpu.py).

Keys come from msig_keyset_cases.key_set(): 12 valid keys with known secret keys, then the identity, the order-2 point, an
order-8 point and a valid key with q added to its u coordinate.  A `VCase` is one call in both forms at once: the inline key
column `PK` (what the code under test gets), `PK_clean` (the same with the keys of refused vectors put back: what the oracle
gets), the index column `key_idx`, the offsets, and one (u, R, m) per vector.  A vector is signed with the aggregate secret
sum d_i sk_i mod r through jjs_oracle_c.sign_single when all its keys are among the 12, and `build` asserts that the key that
call returns is the oracle's aggregate -- which checks this builder, not the engine.

Expected values (`expected`): the aggregates are jjs_oracle_c.multisig_combine's agg_pk on PK_clean with canonical dummy share
columns (z = 0, m = 0, R = S = the identity; its agg_pk does not depend on them), the statuses jjs_oracle_c.verify_single's on
that aggregate; an empty vector has the identity for an aggregate, a refused vector zeros, vec_status 3 and status 3 (the
fixed definitions of include/jjs_gpu.h).  Nothing is off the curve or out of range outside the refusal cases and the three
encodings the verification itself rejects (u >= r, m >= q, an R coordinate >= q: jjs_oracle_c.verify_single gives 3 for them).
"""
from __future__ import annotations

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc
import msig_ext_cases as xc
import msig_keyset_cases as kcs
import multisig_cases as mc
from helpers import pt_bytes, torsion_generator

IDENT = pt_bytes(o.IDENTITY)
INLINE_REFUSALS = ("u coordinate >= q", "v coordinate = q", "off the curve")
KEYSET_REFUSALS = kcs.REFUSALS + (("non-canonical", kcs.NONCANONICAL_KEY),)


class VCase:
    def __init__(self, PK, key_idx, offsets, u, R, m, PK_clean=None, refused=None, where=None):
        self.PK = np.array(PK, np.uint8, order="C").reshape(-1, 64)
        self.PK_clean = np.array(self.PK if PK_clean is None else PK_clean, np.uint8, order="C").reshape(-1, 64)
        self.key_idx = np.array(key_idx, np.uint32).reshape(-1)
        self.offsets = np.array(offsets, np.int64)
        self.u, self.R, self.m = (np.array(x, np.uint8, order="C").reshape(-1, w) for x, w in ((u, 32), (R, 64), (m, 32)))
        self.refused = dict(refused or {})          # vector -> cause
        self.where = dict(where or {})              # name -> vector
        assert len(self.PK) == len(self.key_idx) == self.n and len(self.u) == len(self.R) == len(self.m) == self.B

    @property
    def n(self):
        return int(self.offsets[-1])

    @property
    def B(self):
        return len(self.offsets) - 1

    def offs32(self):
        return self.offsets.astype(np.uint32)

    def sizes(self):
        return np.diff(self.offsets)

    def row(self, t, j):
        assert 0 <= j < self.offsets[t + 1] - self.offsets[t], (t, j)
        return int(self.offsets[t]) + j

    def usable(self):
        ok = np.ones(self.B, bool)
        ok[list(self.refused)] = False
        return ok

    # ---- the signature of a vector ----
    def spoil_u(self, t):
        self.u[t] = mc._fe([(mc._ints(self.u[t:t + 1])[0] + 1) % o.R_ORDER])[0]

    def set_R(self, t, point):
        self.R[t] = pt_bytes(point)

    # ---- refusals ----
    def refuse_inline(self, t, j, cause):
        i = self.row(t, j)
        u, v = (int.from_bytes(self.PK[i, k:k + 32].tobytes(), "little") for k in (0, 32))
        if cause == "u coordinate >= q":
            assert u + o.Q < 1 << 256
            self.PK[i, :32] = mc._fe([u + o.Q])[0]
        elif cause == "v coordinate = q":
            self.PK[i, 32:] = mc._fe([o.Q])[0]
        else:
            assert cause == "off the curve"
            self.PK[i, 32:] = mc._fe([(v + 1) % o.Q])[0]
            assert not oc.point_flags(self.PK[i:i + 1])[0] & 1, "the planted point is on the curve"
        self.refused[t] = cause

    def refuse_keyset(self, t, j, index, cause):
        self.key_idx[self.row(t, j)] = index
        self.refused[t] = cause


def concat(*cs) -> VCase:
    offs, refused, where, n, B = [np.zeros(1, np.int64)], {}, {}, 0, 0
    for c in cs:
        offs.append(c.offsets[1:] + n)
        refused.update({t + B: w for t, w in c.refused.items()})
        where.update({k: t + B for k, t in c.where.items()})
        n += c.n; B += c.B
    cat = lambda k: np.concatenate([getattr(c, k) for c in cs])  # noqa: E731
    return VCase(cat("PK"), cat("key_idx"), np.concatenate(offs), cat("u"), cat("R"), cat("m"), cat("PK_clean"), refused, where)


def tile(c: VCase, reps: int) -> VCase:
    offs = np.concatenate([np.zeros(1, np.int64)] + [c.offsets[1:] + r * c.n for r in range(reps)])
    refused = {t + r * c.B: w for r in range(reps) for t, w in c.refused.items()}
    rows = lambda a: np.tile(a, (reps, 1))  # noqa: E731
    return VCase(rows(c.PK), np.tile(c.key_idx, reps), offs, rows(c.u), rows(c.R), rows(c.m), rows(c.PK_clean), refused, c.where)


def build(picks, seed, keys, sk, threads=0) -> VCase:
    """One vector per entry of `picks` (an array of indices into `keys`; an empty one is an empty vector), signed as the module's
    text says; a vector with a key outside the 12 valid ones gets a signature by an unrelated secret key."""
    picks = [np.asarray(p, np.int64).reshape(-1) for p in picks]
    sizes = [len(p) for p in picks]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, B = int(offs[-1]), len(sizes)
    flat = np.concatenate(picks + [np.zeros(0, np.int64)])
    rng = np.random.default_rng(seed)
    PK = keys[flat] if N else np.zeros((0, 64), np.uint8)
    d = [0] * N
    by_n = {}
    for t, n in enumerate(sizes):
        if n:
            by_n.setdefault(n, []).append(t)
    for n, ts in by_n.items():                                # d_i = H(pk_i, pk_lo .. pk_hi)
        idx = offs[np.array(ts)][:, None] + np.arange(n)[None, :]
        pk = PK[idx]
        pre = np.empty((len(ts), n, 2 + 2 * n, 32), np.uint8)
        pre[:, :, 0] = pk[:, :, :32]; pre[:, :, 1] = pk[:, :, 32:]
        pre[:, :, 2::2] = pk[:, None, :, :32]; pre[:, :, 3::2] = pk[:, None, :, 32:]
        for i, v in zip(idx.reshape(-1), mc._ints(oc.poseidon_any(pre.reshape(-1, 2 + 2 * n, 32), threads))):
            d[int(i)] = v & mc.MASK250
    signed = np.array([n > 0 and bool((p < len(sk)).all()) for n, p in zip(sizes, picks)], bool)
    agg_sk = []
    for t in range(B):
        lo, hi = int(offs[t]), int(offs[t + 1])
        agg_sk.append(sum(d[i] * sk[int(flat[i])] for i in range(lo, hi)) % o.R_ORDER if signed[t] else 0)
    other = mc._scalars(rng, B)
    agg_sk = [a if a else x for a, x in zip(agg_sk, other)]   # (an aggregate secret of 0 would be the identity: not signed with)
    m = rng.integers(0, 256, (B, 32), dtype=np.uint8)
    m[:, 31] &= 0x3F                                          # < 2^254 < q
    u, R, PKs = oc.sign_single(mc._fe(agg_sk), mc._fe(mc._scalars(rng, B)), m, threads)
    c = VCase(PK, flat, offs, u, R, m)
    if signed.any():
        assert (PKs[signed] == oracle_aggregates(c, threads)[signed]).all(), "the builder's aggregate secret is not the oracle's aggregate key"
    return c


def oracle_aggregates(c: VCase, threads=0):
    """aggregate_pk of every vector of PK_clean by the oracle; the identity for an empty one.  (Computed once per case: PK_clean
    does not change when a vector is refused or a signature spoilt.)"""
    if getattr(c, "_agg", None) is not None:
        return c._agg.copy()
    agg = np.tile(IDENT, (c.B, 1))
    if c.n:
        ident = np.tile(IDENT, (c.n, 1))
        got = oc.multisig_combine(np.zeros((c.n, 32), np.uint8), c.PK_clean, ident, ident, np.zeros((c.B, 32), np.uint8), c.offs32(),
                                  threads=threads)[2]
        full = c.sizes() > 0
        agg[full] = got[full]
    c._agg = agg.copy()
    return agg


def expected(c: VCase, threads=0, derived_R=None):
    """(agg_pk, vec_status, status, tally) of the call; derived_R: the derived affine column of an extended R."""
    ok = c.usable()
    agg = oracle_aggregates(c, threads)
    st = oc.verify_single(c.u, c.R if derived_R is None else derived_R, agg, c.m, threads).copy()
    agg[~ok] = 0
    st[~ok] = 3
    vst = np.where(ok, 0, 3).astype(np.uint8)
    return agg, vst, st.astype(np.uint8), np.bincount(st, minlength=4).astype(np.uint64)


def draw(rng, n):
    return rng.permutation(kcs.N_VALID)[:n] if n <= kcs.N_VALID else rng.integers(0, kcs.N_VALID, n)


def standard_mix(keys, sk, form: str, seed: int = 1200, threads: int = 0, T: int = 100) -> VCase:
    """About T vectors and 3.5 T key rows: sizes 1, 2, 3 and 8; one key twice in a vector; an empty vector; (inline) a vector
    holding the order-2 point beside valid keys, whose aggregate has a torsion part; a spoilt u; R the identity and R of small
    order; u >= r, m >= q and an R coordinate >= q; one refused vector per cause of the form, each between two good ones."""
    assert form in ("inline", "keyset")
    rng = np.random.default_rng(seed)
    picks, where = [], {}

    def add(name, p):
        if name:
            where[name] = len(picks)
        picks.append(np.asarray(p, np.int64))

    for n in (1, 2, 3, 8):
        add(f"good {n}", draw(rng, n))
    add("same key twice", [5, 2, 5])
    add("empty", [])
    if form == "inline":
        add("torsion", [3, kcs.ORDER2_KEY, 7])
        add("identity key", [kcs.IDENTITY_KEY, 4])
        add("only the identity", [kcs.IDENTITY_KEY])
        add("order 8 key", [1, kcs.ORDER8_KEY])
    for name, n in (("spoilt u", 3), ("R identity", 2), ("R small order", 2), ("u >= r", 2), ("m >= q", 3), ("R.v >= q", 2), ("", 2)):
        add(name, draw(rng, n))
    causes = INLINE_REFUSALS if form == "inline" else [w for w, _ in KEYSET_REFUSALS]
    for cause in causes:
        add(cause, draw(rng, 3))
        add("", draw(rng, 2))
    k = 0
    while len(picks) < T:
        add("", draw(rng, (1, 2, 3, 8)[k % 4])); k += 1
    c = build(picks, seed + 1, keys, sk, threads)
    c.where = where
    c.spoil_u(where["spoilt u"])
    c.set_R(where["R identity"], o.IDENTITY)
    c.set_R(where["R small order"], torsion_generator())
    c.u[where["u >= r"]] = mc._fe([o.R_ORDER])[0]
    c.m[where["m >= q"]] = mc._fe([o.Q])[0]
    c.R[where["R.v >= q"], 32:] = mc._fe([o.Q])[0]
    if form == "inline":
        for k, cause in enumerate(INLINE_REFUSALS):
            c.refuse_inline(where[cause], k % 3, cause)
    else:
        for k, (cause, index) in enumerate(KEYSET_REFUSALS):
            c.refuse_keyset(where[cause], k % 3, index, cause)
    return c


def check_named(c: VCase, form: str, agg, st, label=""):
    """What the named vectors of the standard mix must give, written out without the oracle."""
    w = c.where
    for name in ("good 1", "good 2", "good 3", "good 8", "same key twice"):
        assert st[w[name]] == 0 and agg[w[name]].any(), (label, name)
    assert st[w["empty"]] == 1 and (agg[w["empty"]] == IDENT).all(), (label, "empty")
    assert st[w["spoilt u"]] == 2, label
    for name in ("R identity", "R small order"):
        assert st[w[name]] == 1, (label, name)
    for name in ("u >= r", "m >= q", "R.v >= q"):
        assert st[w[name]] == 3 and agg[w[name]].any(), (label, name)
    if form == "inline":
        for name in ("torsion", "identity key", "only the identity", "order 8 key"):
            assert agg[w[name]].any() and c.refused.get(w[name]) is None, (label, name)
        assert st[w["torsion"]] == 1 and st[w["only the identity"]] == 1 and (agg[w["only the identity"]] == IDENT).all(), label
    for t, cause in c.refused.items():
        assert st[t] == 3 and not agg[t].any(), (label, cause)
        assert st[t - 1] == 0 and st[t + 1] == 0 and agg[t - 1].any() and agg[t + 1].any(), (label, cause, "the neighbours")


def ragged(rows: int, seed: int, keys, sk, form: str, threads: int = 0, refusals: int = 3) -> VCase:
    """`rows` key rows in ragged vectors of 1 to 8 keys, a spoilt signature in every seventh, and a few refusals."""
    rng = np.random.default_rng(seed)
    c = build([draw(rng, n) for n in mc.ragged_sizes(rng, rows)], seed + 1, keys, sk, threads)
    for t in range(3, c.B, 7):
        c.spoil_u(t)
    for k, t in enumerate(np.linspace(5, c.B - 2, refusals).astype(int)):
        j = int(c.sizes()[t]) - 1
        if form == "inline":
            c.refuse_inline(int(t), j, INLINE_REFUSALS[k % 3])
        else:
            c.refuse_keyset(int(t), j, *KEYSET_REFUSALS[k % len(KEYSET_REFUSALS)][::-1])
    return c


# ---- the extended format -------------------------------------------------------------------------------------------------
class ExtV:
    """The extended columns of a VCase (PK and R as U || V || Z with random Z, the first rows Z = 1, q - 1, 2) with unusable
    points planted: a key whose coordinate was >= q becomes U = q, and `plant_key` / `plant_R` make further points unusable.
    `case` is the derived affine call (an unusable key refuses its vector), `derived_R` the derived R column."""

    def __init__(self, c: VCase, seed: int):
        rng = np.random.default_rng(seed)
        self.case = VCase(c.PK, c.key_idx, c.offsets, c.u, c.R, c.m, c.PK_clean, c.refused, c.where)
        self.case._agg = getattr(c, "_agg", None)
        canon = c.R.copy()
        bad_R = [t for t in range(c.B) if any(int.from_bytes(c.R[t, k:k + 32].tobytes(), "little") >= o.Q for k in (0, 32))]
        canon[bad_R] = IDENT
        self.R = xc.to_ext_column(canon, rng, xc.CHOSEN_Z)
        for t in bad_R:
            xc.spoil(self.R[t], "V=q+1")
        src = c.PK.copy()
        bad_pk = [i for i in range(c.n) if any(int.from_bytes(c.PK[i, k:k + 32].tobytes(), "little") >= o.Q for k in (0, 32))]
        src[bad_pk] = c.PK_clean[bad_pk]
        self.PK = xc.to_ext_column(src, rng, xc.CHOSEN_Z[1:])
        for i in bad_pk:
            xc.spoil(self.PK[i], "U=q")
        self.derived_R = xc.derive_column(self.R)

    def plant_key(self, t, j, kind):
        xc.spoil(self.PK[self.case.row(t, j)], kind)
        self.case.refused[t] = "key " + kind

    def plant_R(self, t, kind):
        xc.spoil(self.R[t], kind)
        self.derived_R[t] = 0xFF


def ext_mix(keys, sk, form: str, seed: int = 1300, threads: int = 0, T: int = 40):
    """The standard mix in the extended format with Z != 1 rows, a Z = 0 key (inline) and a Z = 0 R."""
    c = standard_mix(keys, sk, form, seed, threads, T)
    x = ExtV(c, seed + 7)
    good = [t for t in range(c.B - 4, c.B)]
    if form == "inline":
        x.plant_key(good[0], 0, "Z=0")
        x.case.where["key Z=0"] = good[0]
    x.plant_R(good[2], "Z=0")
    x.case.where["R Z=0"] = good[2]
    return x

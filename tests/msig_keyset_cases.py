"""Cases for the multisignature call against a registered key set (jjs_multisig_combine_keyset[_dev], csrc/msig_keyset.h),
shared by the CPU build (test_msig_keyset_host.py) and the device (test_msig_keyset_gpu.py).

The key set has 16 keys: 12 valid ones with known secret keys, then the identity, the order-2 point, an order-8 point (status 1
each) and a valid key with q added to its u coordinate (non-canonical: status 3).  A `KsCase` is a `multisig_cases.Case` whose
PK column holds the registered bytes of the keys its shares were signed with, plus the index column the call under test takes.
`pool_transcripts` is multisig_cases.valid_transcripts with the secret key of every share drawn from the set's 12 instead of
afresh (valid_transcripts takes no keys, so its signing steps are restated here over its own helpers; the oracle, not this
builder, says whether a share is valid: multisig_cases.expected asserts the plan).  `refuse` then points a row at an unusable
key: the expected outputs of that transcript are the fixed definition of include/jjs_gpu.h (every share 3, transcript 3,
agg_pk / sig_u / sig_R zero), those of every other transcript stay the oracle's.
"""
from __future__ import annotations

import copy

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc
import multisig_cases as mc
from helpers import pt_bytes, torsion_generator

N_VALID = 12
IDENTITY_KEY, ORDER2_KEY, ORDER8_KEY, NONCANONICAL_KEY = 12, 13, 14, 15
KEY_STATUS = [0] * N_VALID + [1, 1, 1, 3]
REFUSALS = (("index == n_keys", 16), ("index 0xFFFFFFFF", 0xFFFFFFFF), ("identity", IDENTITY_KEY), ("order 2", ORDER2_KEY),
            ("order 8", ORDER8_KEY))


def key_set(seed: int = 900):
    """(keys (16, 64) uint8, the 12 secret keys)."""
    rng = np.random.default_rng(seed)
    sk = mc._scalars(rng, N_VALID + 1)
    G = np.tile(pt_bytes(o.G), (N_VALID + 1, 1))
    pts = oc.scalar_mul(G, mc._fe(sk))
    bad = pts[N_VALID].copy()
    u = int.from_bytes(bad[:32].tobytes(), "little")
    assert u + o.Q < 1 << 256
    bad[:32] = mc._fe([u + o.Q])[0]
    keys = np.concatenate([pts[:N_VALID], np.stack([pt_bytes(o.IDENTITY), pt_bytes(o.ORDER2), pt_bytes(torsion_generator()), bad])])
    return np.ascontiguousarray(keys, np.uint8), sk[:N_VALID]


class KsCase:
    def __init__(self, case: mc.Case, key_idx, refused=None):
        self.case = case
        self.key_idx = np.array(key_idx, np.uint32)
        self.refused = dict(refused or {})            # transcript -> what
        assert len(self.key_idx) == case.n

    @property
    def T(self):
        return self.case.T

    def refuse(self, t, j, index, what=""):
        """Row j of transcript t names `index` (outside the set, or a key whose status is not 0)."""
        self.key_idx[self.case.row(t, j)] = index
        self.refused[t] = what

    def args(self):
        """key_idx, z, R, S, m, offsets of the call under test."""
        d = self.case.dirty
        return self.key_idx, d["z"], d["R"], d["S"], d["m"], self.case.offsets.astype(np.uint32)

    def inline_args(self):
        """z, PK, R, S, m, offsets of the inline call on the gathered column (the signing keys: rows of refused transcripts too)."""
        return self.case.args()

    def usable(self):
        """Per transcript: no row of it is unusable."""
        ok = np.ones(self.T, bool)
        ok[list(self.refused)] = False
        return ok


def concat(*kcs) -> KsCase:
    refused, T = {}, 0
    for kc in kcs:
        refused.update({t + T: w for t, w in kc.refused.items()})
        T += kc.T
    return KsCase(mc.concat(*[kc.case for kc in kcs]), np.concatenate([kc.key_idx for kc in kcs]), refused)


def pool_transcripts(sizes, seed, keys, sk_pool, picks=None, threads=0) -> KsCase:
    """Valid transcripts of the given participant counts whose signers are ordered draws (with repetition across transcripts, and
    where `picks` says so inside one) from the set's valid keys."""
    sizes = [int(x) for x in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, T = int(offs[-1]), len(sizes)
    rng = np.random.default_rng(seed)
    nv = len(sk_pool)                                         # the set's valid keys come first
    if picks is None:
        picks = np.concatenate([rng.permutation(nv)[:n] if n <= nv else rng.integers(0, nv, n) for n in sizes] +
                               [np.zeros(0, np.int64)]).astype(np.int64)
    picks = np.asarray(picks, np.int64)
    assert len(picks) == N and (picks < nv).all()
    sk = [sk_pool[int(k)] for k in picks]
    r, s = (mc._scalars(rng, N) for _ in range(2))
    m = rng.integers(0, 256, (T, 32), dtype=np.uint8)
    m[:, 31] &= 0x3F
    G = np.tile(pt_bytes(o.G), (max(N, T, 1), 1))
    PK = keys[picks] if N else np.zeros((0, 64), np.uint8)
    R, S = (oc.scalar_mul(G[:N], mc._fe(v), threads) for v in (r, s))
    span = lambda v, t: v[int(offs[t]):int(offs[t + 1])]  # noqa: E731
    d, a = [0] * N, [0] * T
    AGG = np.zeros((T, 64), np.uint8)
    by_n = {}
    for t, n in enumerate(sizes):
        if n:
            by_n.setdefault(n, []).append(t)
    by_n = {n: (np.array(ts), offs[np.array(ts)][:, None] + np.arange(n)[None, :]) for n, ts in by_n.items()}
    for n, (ts, idx) in by_n.items():                         # d_i = H(pk_i, pk_lo .. pk_hi)
        pk = PK[idx]
        pre = np.empty((len(ts), n, 2 + 2 * n, 32), np.uint8)
        pre[:, :, 0] = pk[:, :, :32]; pre[:, :, 1] = pk[:, :, 32:]
        pre[:, :, 2::2] = pk[:, None, :, :32]; pre[:, :, 3::2] = pk[:, None, :, 32:]
        for i, v in zip(idx.reshape(-1), mc._ints(oc.poseidon_any(pre.reshape(-1, 2 + 2 * n, 32), threads))):
            d[int(i)] = v & mc.MASK250
    AGG = oc.scalar_mul(G[:T], mc._fe([sum(x * k for x, k in zip(span(d, t), span(sk, t))) % o.R_ORDER for t in range(T)]), threads)
    for n, (ts, idx) in by_n.items():                         # a = H(pk_agg, m, R_lo, S_lo, ...)
        pre = np.empty((len(ts), 3 + 4 * n, 32), np.uint8)
        pre[:, 0] = AGG[ts, :32]; pre[:, 1] = AGG[ts, 32:]; pre[:, 2] = m[ts]
        pre[:, 3::4] = R[idx][:, :, :32]; pre[:, 4::4] = R[idx][:, :, 32:]
        pre[:, 5::4] = S[idx][:, :, :32]; pre[:, 6::4] = S[idx][:, :, 32:]
        for t, v in zip(ts, mc._ints(oc.poseidon_any(pre, threads))):
            a[int(t)] = v & mc.MASK250
    RSA = oc.scalar_mul(G[:T], mc._fe([(sum(span(r, t)) + a[t] * sum(span(s, t))) % o.R_ORDER for t in range(T)]), threads)
    c5 = np.stack([RSA[:, :32], RSA[:, 32:], AGG[:, :32], AGG[:, 32:], m], 1) if T else np.zeros((0, 5, 32), np.uint8)
    c = [v & mc.MASK250 for v in mc._ints(oc.poseidon(c5, threads))]
    z = []
    for t in range(T):
        z += [(ri + si * a[t] - c[t] * di * ki) % o.R_ORDER for ri, si, di, ki in zip(span(r, t), span(s, t), span(d, t), span(sk, t))]
    return KsCase(mc.Case({"z": mc._fe(z), "PK": PK, "R": R, "S": S, "m": m}, offs, np.zeros(N, np.int16)), picks)


def host_mix(keys, sk, seed: int = 910, threads: int = 0, coord: bool = False):
    """The host harness's cases in one call: transcripts of 1, 2, 3 and 8 participants (one of 3 names the same key twice), a
    spoilt share in front of a z >= r (status 4, then 3: the first failure decides), z >= r alone, an empty transcript, and one
    refused transcript per cause of REFUSALS, each between two good ones.  coord: also an R coordinate >= q at the first share
    of a transcript (the oracle does not define the rest of that transcript: compare with the inline passes).
    Returns the case and {what: transcript}."""
    sizes = [1, 2, 3, 8, 3, 4, 3, 0, 2]
    picks = None
    rng = np.random.default_rng(seed)
    draw = lambda n: rng.permutation(N_VALID)[:n]  # noqa: E731
    picks = [draw(n) for n in sizes]
    picks[4] = np.array([5, 2, 5])                              # one key twice in one transcript
    where = {"good 1": 0, "good 2": 1, "good 3": 2, "good 8": 3, "same key twice": 4, "spoilt then z >= r": 5, "z >= r": 6, "empty": 7}
    for what, _ in REFUSALS:
        where[what] = len(sizes)
        sizes += [3, 2]
        picks += [draw(3), draw(2)]
    if coord:
        where["R.v >= q"] = len(sizes)
        sizes += [3, 1]
        picks += [draw(3), draw(1)]
    kc = pool_transcripts(sizes, seed + 1, keys, sk, np.concatenate(picks), threads)
    kc.case.corrupt(where["spoilt then z >= r"], 1); kc.case.bad_z(where["spoilt then z >= r"], 3, o.R_ORDER)
    kc.case.bad_z(where["z >= r"], 1, mc.ALL_ONES)
    for k, (what, index) in enumerate(REFUSALS):
        kc.refuse(where[what], k % 3, index, what)
    if coord:
        kc.case.bad_coord(where["R.v >= q"], 0, "R", 1, o.Q)
    return kc, where


def expected(kc: KsCase, threads: int = 0) -> mc.Expected:
    """multisig_cases.expected (the oracle on the signing keys) with the fixed definition written over the refused transcripts."""
    e = copy.copy(mc.expected(kc.case, threads))
    for k in ("st", "ts", "agg", "su", "sr", "cmp_share", "cmp_agg", "ts_exact"):
        setattr(e, k, getattr(e, k).copy())
    for t in kc.refused:
        lo, hi = int(kc.case.offsets[t]), int(kc.case.offsets[t + 1])
        e.st[lo:hi] = 3; e.ts[t] = 3; e.agg[t] = 0; e.su[t] = 0; e.sr[t] = 0
        e.cmp_share[lo:hi] = True; e.cmp_agg[t] = True; e.ts_exact[t] = True
    e.uncompared = int((~e.cmp_share).sum())
    return e


def check_against_inline(kc: KsCase, got, inline, label: str = ""):
    """Byte for byte: the usable transcripts against the inline call's outputs on the gathered column, the refused ones
    against the fixed definition.  got, inline = (share_status, agg_pk, sig_u, sig_R, transcript_status or None)."""
    ok_t = kc.usable()
    ok_s = np.repeat(ok_t, kc.case.sizes())
    names = ("share_status", "agg_pk", "sig_u", "sig_R", "transcript_status")
    for name, g, w in zip(names, got, inline):
        if g is None or w is None:
            assert name == "transcript_status", (label, name)
            continue
        mask = ok_s if name == "share_status" else ok_t
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        diff = (g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(1) & mask
        assert not diff.any(), (label, name, np.nonzero(diff)[0][:8].tolist())
        if name in ("share_status", "transcript_status"):
            assert (g[~mask] == 3).all(), (label, name, "a refused transcript")
        else:
            assert not g[~mask].any(), (label, name, "a refused transcript keeps an output")


def to_ext(pts, seed: int = 1):
    """(n, 64) affine -> (n, 96) U || V || Z with Z = 1."""
    pts = np.ascontiguousarray(pts, np.uint8)
    out = np.zeros((len(pts), 96), np.uint8)
    out[:, :64] = pts
    out[:, 64] = 1
    return out

"""Cases for the multisig signer groups (jjs_msig_group_*, csrc/msig_group.h), shared by the CPU build
(test_msig_group_host.py) and the device (test_msig_group_gpu.py).

A `GroupCase` is a key vector of n participants and a `multisig_cases.Case` of T transcripts of exactly these participants in
the TILED INLINE FORM: PK repeated T times, offsets[t] = t n.  Expected values are `multisig_cases.expected` of that case, that
is jjs_oracle_c.multisig_combine on the inline form -- never the code under test -- and `multisig_cases.check` compares, with
the group's aggregate key repeated per transcript standing in for the inline call's agg_pk rows.

Inputs are signed with known secret keys as multisig_cases.valid_transcripts signs them; the key vector is drawn once per
group, d_i and the aggregate key are computed once.  A participant's secret key may be 0 (PK = identity, the shares stay valid)
or equal to another's (the same key twice, valid as well); `with_point` puts an identity / order-2 / order-8 point in place of
a key the way multisig_cases.small_order_case does: the shares stay as signed, every hash changes, the oracle decides.
"""
from __future__ import annotations

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc
import multisig_cases as mc
from helpers import pt_bytes

ALL_ONES = mc.ALL_ONES


class GroupCase:
    def __init__(self, PK: np.ndarray, case: mc.Case):
        self.PK = np.ascontiguousarray(PK, np.uint8)
        self.case = case
        self.n = len(self.PK)
        assert case.T * self.n == case.n and (case.sizes() == self.n).all()
        assert (case.clean["PK"].reshape(case.T, self.n, 64) == self.PK[None]).all() and (case.dirty["PK"] == case.clean["PK"]).all()
        assert not any(col == "PK" for _, kind, _, col in case.marks if kind == "coord"), "a group's keys are range-checked at registration"

    @property
    def T(self):
        return self.case.T

    def call_args(self):
        """z, R, S, m of the group call (the rows of the inline form, without PK and offsets)."""
        d = self.case.dirty
        return d["z"], d["R"], d["S"], d["m"]

    def slice(self, t0, t1) -> "GroupCase":
        return GroupCase(self.PK, self.case.slice(t0, t1))

    def tile(self, reps) -> "GroupCase":
        return GroupCase(self.PK, mc.tile(self.case, reps))


def as_inline_outputs(gc: GroupCase, agg_pk, got):
    """(share_status, sig_u, sig_R, transcript_status) of a group call + the group's key -> the tuple multisig_cases.check takes."""
    st, su, sr, ts = got
    return st, np.tile(np.asarray(agg_pk, np.uint8).reshape(1, 64), (gc.T, 1)), su, sr, ts


def group_transcripts(n: int, T: int, seed: int, zero_sk=(), same_sk=(), threads: int = 0) -> GroupCase:
    """T valid transcripts of one group of n participants.  zero_sk: participants whose secret key is 0 (PK = identity);
    same_sk = [(j, k)]: participant j signs with participant k's key (the same key twice)."""
    rng = np.random.default_rng(seed)
    sk = mc._scalars(rng, n)
    for j in zero_sk:
        sk[j] = 0
    for j, k in same_sk:
        sk[j] = sk[k]
    N = n * T
    r, s = mc._scalars(rng, N), mc._scalars(rng, N)
    m = rng.integers(0, 256, (T, 32), dtype=np.uint8)
    m[:, 31] &= 0x3F
    G = np.tile(pt_bytes(o.G), (max(N, 1), 1))
    PK = oc.scalar_mul(G[:n], mc._fe(sk), threads)
    R, S = oc.scalar_mul(G[:N], mc._fe(r), threads), oc.scalar_mul(G[:N], mc._fe(s), threads)
    pre = np.empty((n, 2 + 2 * n, 32), np.uint8)                     # d_i = H(pk_i, pk_1 .. pk_n)
    pre[:, 0] = PK[:, :32]; pre[:, 1] = PK[:, 32:]
    pre[:, 2::2] = PK[None, :, :32]; pre[:, 3::2] = PK[None, :, 32:]
    d = [v & mc.MASK250 for v in mc._ints(oc.poseidon_any(pre, threads))]
    agg = oc.scalar_mul(G[:1], mc._fe([sum(x * k for x, k in zip(d, sk)) % o.R_ORDER]), threads)[0]
    Rt, St = R.reshape(T, n, 64), S.reshape(T, n, 64)
    pre = np.empty((T, 3 + 4 * n, 32), np.uint8)                     # a = H(pk_agg, m, R_1, S_1, ...)
    pre[:, 0] = agg[:32]; pre[:, 1] = agg[32:]; pre[:, 2] = m
    pre[:, 3::4] = Rt[:, :, :32]; pre[:, 4::4] = Rt[:, :, 32:]; pre[:, 5::4] = St[:, :, :32]; pre[:, 6::4] = St[:, :, 32:]
    a = [v & mc.MASK250 for v in mc._ints(oc.poseidon_any(pre, threads))]
    span = lambda v, t: v[t * n:(t + 1) * n]  # noqa: E731
    RSA = oc.scalar_mul(G[:T], mc._fe([(sum(span(r, t)) + a[t] * sum(span(s, t))) % o.R_ORDER for t in range(T)]), threads)
    c5 = np.stack([RSA[:, :32], RSA[:, 32:], np.tile(agg[:32], (T, 1)), np.tile(agg[32:], (T, 1)), m], 1)
    c = [v & mc.MASK250 for v in mc._ints(oc.poseidon(c5, threads))]
    z = []
    for t in range(T):
        z += [(ri + si * a[t] - c[t] * di * ki) % o.R_ORDER for ri, si, di, ki in zip(span(r, t), span(s, t), d, sk)]
    case = mc.Case({"z": mc._fe(z), "PK": np.tile(PK, (T, 1)), "R": R, "S": S, "m": m}, np.arange(T + 1, dtype=np.int64) * n, np.zeros(N, np.int16))
    return GroupCase(PK, case)


def with_point(gc: GroupCase, j: int, point) -> GroupCase:
    """The same shares under a key vector whose participant j is `point` (on the curve): nothing is planned any more."""
    PK = gc.PK.copy()
    PK[j] = pt_bytes(point)
    c = gc.case
    clean = {k: c.clean[k] for k in mc.COLS}
    dirty = {k: c.dirty[k] for k in mc.COLS}
    clean["PK"] = dirty["PK"] = np.tile(PK, (c.T, 1))
    return GroupCase(PK, mc.Case(clean, c.offsets, np.full(c.n, -1, np.int16), dirty, c.marks))


def mix(gc: GroupCase, coord=()) -> list:
    """The issue's mix written into gc's transcripts, from transcript 1 on (0 stays valid), as far as the group's size allows:
    a corrupted z at the first, a middle and the last slot; two bad shares in one transcript (both orders of 3 and 4); z >= r;
    m >= q; then one transcript per entry of `coord` = [("R" | "S", half, value)] with that coordinate out of range.
    Returns [(t, what)]; the transcripts behind the last one stay valid."""
    c, n, t, done = gc.case, gc.n, 1, []

    def take(what):
        nonlocal t
        assert t < c.T, "the case has too few transcripts for the mix"
        done.append((t, what)); t += 1
        return t - 1
    for where in mc.POSITIONS if n > 2 else mc.POSITIONS[:n]:
        c.corrupt(take(f"corrupt {where}"), mc._pos(n, where))
    if n >= 2:
        k = take("two bad shares: 4 then 3"); c.corrupt(k, 0); c.bad_z(k, n - 1, o.R_ORDER)
        k = take("two bad shares: 3 then 4"); c.bad_z(k, 0 if n == 2 else n // 2 - 1, ALL_ONES); c.corrupt(k, n - 1)
        k = take("two invalid shares"); c.corrupt(k, 0); c.corrupt(k, n - 1)
    c.bad_z(take("z = r"), n // 2, o.R_ORDER)
    c.bad_m(take("m = q"), o.Q)
    for col, half, value in coord:
        c.bad_coord(take(f"{col}.{'uv'[half]} >= q"), n - 1, col, half, value)
    return done


def torsion_key_case(seed: int = 400, T: int = 3) -> GroupCase:
    """A group of two whose first key carries a small-order part, PK_0 = sk_0 G + T8 (T8 of order 8), and transcripts the
    REFERENCE accepts: signer 0 commits to R_0 = r_0 G + X with X = (c d_0 mod r) T8, found by trying the eight multiples of T8
    until the transcript's own challenge agrees, so that z_0 G + (c d_0 mod r) PK_0 == R_0 + a S_0 holds.  The reference reduces
    c d_0 mod r before it multiplies; c (d_0 PK_0) has the small-order part (c d_0 as integers) T8 instead, which differs."""
    from helpers import torsion_generator
    rng = np.random.default_rng(seed)
    t8 = torsion_generator()
    sk = mc._scalars(rng, 2)
    pks = [o.add(o.mul(o.G, sk[0]), t8), o.mul(o.G, sk[1])]
    z, R, S, m = [], [], [], []
    unreduced_differs = False
    while len(m) < T:
        r, s = mc._scalars(rng, 2), mc._scalars(rng, 2)
        msg = int(rng.integers(1, 1 << 62))
        Ss = [o.mul(o.G, x) for x in s]
        for k in range(8):
            Rs = [o.add(o.mul(o.G, r[0]), o.mul(t8, k)), o.mul(o.G, r[1])]
            ds, _, a, _, c = o.multisig_transcript(pks, Rs, Ss, msg)
            e = c * ds[0] % o.R_ORDER
            if e % 8 == k:
                unreduced_differs |= (c * ds[0]) % 8 != k
                z += [(r[0] + s[0] * a - e * sk[0]) % o.R_ORDER, (r[1] + s[1] * a - c * ds[1] * sk[1]) % o.R_ORDER]
                R += Rs; S += Ss; m.append(msg)
                break
    assert unreduced_differs, "no transcript tells the reduced product from the unreduced one: another seed"
    PK = np.stack([pt_bytes(p) for p in pks])
    pts = lambda ps: np.stack([pt_bytes(p) for p in ps])  # noqa: E731
    case = mc.Case({"z": mc._fe(z), "PK": np.tile(PK, (len(m), 1)), "R": pts(R), "S": pts(S), "m": mc._fe(m)},
                   np.arange(len(m) + 1, dtype=np.int64) * 2, np.zeros(2 * len(m), np.int16))
    return GroupCase(PK, case)

"""The wire forms of the multisignature calls on the CPU: msig_decode_lane (csrc/decode.h), the lane body of
msig_decode_kernel, against derived columns computed in Python integers (msig_wire_cases.py), with launch shapes in which one
lane owns several points, with one, two and three sources and with a strided source; then whole calls -- that lane body in front
of the CPU build of the passes -- against jjs_oracle_c.multisig_combine on the derived columns through multisig_cases.check,
inline, by group and by key set, the verifier's calls against msig_verify_cases.expected, and the reference's multisignature
known answer from its wire bytes."""
import json
import os

import numpy as np
import pytest

import hostlib as hl
import jjs_oracle as o
import msig_group_cases as gcs
import msig_group_hostlib as gh
import msig_keyset_cases as kcs
import msig_keyset_hostlib as kl
import msig_verify_cases as vc
import msig_verify_hostlib as vl
import msig_wire_cases as wc
import msig_wire_hostlib as wh
import multisig_cases as mc


def planted_call():
    """210 shares in ragged transcripts, every kind in every column (msig_wire_cases.plant_everywhere)."""
    x = wc.WireCase(mc.filler(210, seed=31, top=5))
    wc.plant_everywhere(x, boundary=x.T // 2)
    return x


@pytest.fixture(scope="module")
def planted():
    return planted_call()


@pytest.fixture(scope="module")
def keyset():
    return kcs.key_set()


def decoded(x, lanes=64):
    """z, PK, R, S, m, offsets with the wire columns through the lane body."""
    a = x.args()
    return [a[0]] + wh.decode([(x.wire[c], 0) for c in wc.POINT_COLS], lanes=lanes) + a[4:]


def test_the_case_builder_derives_its_columns_from_integers(planted):
    x = planted
    x.check_derived()
    assert len(x.plants) == len(wc.KINDS) * 3 + 1
    for t, j, col, kind in x.plants:
        row = x.derived.dirty[col][x.derived.row(t, j)]
        assert (row == 0xFF).all() == (kind in wc.UNDECODABLE), (t, j, col, kind)
    at = wc.places(x, x.T // 2)
    assert at[0] == (0, 0) and x.derived.row(*at[2]) == x.n - 1 and x.derived.row(*at[3]) + 1 == x.derived.row(*at[4])
    assert 0 < x.derived.row(*at[1]) < x.n - 1
    # both parities of u among the planted decodable points, and the small orders
    pts = {kind: o.decompress(wc.encoding(kind)) for kind in wc.DECODABLE}
    assert pts["odd u"][0] & 1 and not pts["even u"][0] & 1 and pts["identity"] == (0, 1) and pts["order 2"] == (0, o.Q - 1)
    assert pts["order 4 +"][1] == 0 and pts["order 4 -"][1] == 0 and pts["order 4 +"][0] + pts["order 4 -"][0] == o.Q
    nr = int.from_bytes(wc.encoding("non-residue"), "little")
    assert nr < o.Q and pow((nr * nr - 1) * pow(1 + o.D * nr * nr, -1, o.Q) % o.Q, (o.Q - 1) // 2, o.Q) == o.Q - 1


@pytest.mark.parametrize("lanes", [1, 7, 64, 1000])
def test_the_lane_body_gives_the_derived_columns(planted, lanes):
    """lanes = 1: one lane walks every point; 7 and 64: several points per lane, the columns of a row in different lanes; 1000:
    a point per lane and idle lanes.  Then the same points from two sources (a group call's row), from one (a column of the
    verifier's calls), and from a strided source (the R half of u || R rows)."""
    x = planted
    cols = [(x.wire[c], 0) for c in wc.POINT_COLS]
    outs = wh.decode(cols, lanes=lanes)
    for c, got in zip(wc.POINT_COLS, outs):
        diff = np.nonzero((got != x.derived.dirty[c]).any(1))[0]
        assert not len(diff), (c, lanes, diff[:8].tolist())
    outs2 = wh.decode(cols[1:], lanes=lanes)
    outs1 = wh.decode(cols[:1], lanes=lanes)
    assert (outs2[0] == outs[1]).all() and (outs2[1] == outs[2]).all() and (outs1[0] == outs[0]).all()
    sig = wc.sig_rows(np.full((x.n, 32), 0xC3, np.uint8), x.wire["R"])
    strided = wh.decode([(sig, 32)], lanes=lanes)
    assert (strided[0] == outs[1]).all()
    mixed = wh.decode([(x.wire["PK"], 0), (sig, 32)], lanes=lanes)
    assert (mixed[0] == outs[0]).all() and (mixed[1] == outs[1]).all()


def test_every_point_undecodable_and_a_single_row():
    for kind in wc.UNDECODABLE:
        col = np.tile(np.frombuffer(wc.encoding(kind), np.uint8), (5, 1))
        for lanes in (1, 3):
            assert (wh.decode([(col, 0)] * 3, lanes=lanes)[2] == 0xFF).all(), (kind, lanes)
    one = wc.WireCase(mc.valid_transcripts([1], seed=35))
    outs = wh.decode([(one.wire[c], 0) for c in wc.POINT_COLS])
    assert all((got == one.derived.dirty[c]).all() for c, got in zip(wc.POINT_COLS, outs))


def full_call():
    """1601 shares: the six transcripts with undecodable points leave at most 6 x 4 shares uncompared, under 2 % of the call."""
    x = wc.WireCase(mc.filler(1601, seed=41, top=5))
    wc.plant_everywhere(x, boundary=x.T // 3)
    x.derived.bad_z(5, 0, o.R_ORDER)
    return x


def test_combine_inline_against_the_oracle_on_the_derived_columns():
    x = full_call()
    x.check_derived()
    e = mc.expected(x.derived)
    assert 0 < e.uncompared and e.uncompared * 50 < x.n, "the planted points stay within the cap of multisig_cases.check"
    affine = hl.multisig(*x.derived.args())
    got = hl.multisig(*decoded(x, lanes=4096))
    assert mc.check(x.derived, e, got, "wire host") == e.uncompared
    for name, a, b in zip(mc.OUTPUTS, got, affine):
        assert (a == b).all(), name
    st, ts = got[0], got[4]
    for t, j, _, kind in x.plants:
        if kind in wc.UNDECODABLE:
            assert st[x.derived.row(t, j)] == 3 and ts[t] != 0 and not got[2][t].any() and not got[3][t].any(), (t, j, kind)
    # the decodable edge points have no status of their own: what the oracle says about their transcripts, and never 3
    edge = {t for t, _, _, kind in x.plants if kind in wc.DECODABLE}
    assert len(edge) == len(wc.DECODABLE) and all(ts[t] == e.ts[t] and ts[t] != 3 for t in edge)


def test_combine_by_group():
    gc = gcs.group_transcripts(3, 120, seed=53)
    gcs.mix(gc)
    x = wc.WireCase(gc.case)
    x.plant(20, 0, "R", "non-residue"); x.plant(21, 2, "S", "v=q"); x.plant(119, 2, "R", "v=1 signed")
    x.plant(60, 1, "R", "order 4 -"); x.plant(61, 1, "S", "identity")
    x.check_derived()
    rc, keys = wh.decode_keys(wc.compress_column(gc.PK))
    assert rc == 0 and (keys == gc.PK).all(), "a group from wire keys is the group from the keys they decode to"
    gd = gcs.GroupCase(gc.PK, x.derived)
    e = mc.expected(x.derived)
    z, _, R, S, m, _ = decoded(x, lanes=16)
    for by_participant in (False, True):
        rc, got, agg = gh.combine(keys, z, R, S, m, by_participant=by_participant)
        rc2, want, agg2 = gh.combine(gc.PK, *gd.call_args(), by_participant=by_participant)
        assert rc == 0 and rc2 == 0 and (agg == agg2).all()
        for a, b in zip(got, want):
            assert (a == b).all(), by_participant
        mc.check(x.derived, e, gcs.as_inline_outputs(gd, agg, got), f"wire group by_participant={by_participant}")
    assert got[0][x.derived.row(20, 0)] == 3 and got[3][20] == 3 and got[3][21] != 0 and got[3][119] != 0
    assert got[3][60] == e.ts[60] != 3 and got[3][61] == e.ts[61] != 3


@pytest.mark.parametrize("kind", wc.UNDECODABLE)
def test_a_registration_with_an_undecodable_key_is_refused(kind):
    gc = gcs.group_transcripts(3, 2, seed=53)
    pk_w = wc.compress_column(gc.PK)
    assert wh.decode_keys(pk_w)[0] == 0
    for j in (0, 2):
        spoilt = pk_w.copy()
        spoilt[j] = np.frombuffer(wc.encoding(kind), np.uint8)
        assert wh.decode_keys(spoilt)[0] == -1, (kind, j)
    assert wh.decode_keys(pk_w[:0])[0] == -1
    for kind2 in wc.DECODABLE:                    # not validated: a small-order key registers
        edge = pk_w.copy()
        edge[1] = np.frombuffer(wc.encoding(kind2), np.uint8)
        rc, keys = wh.decode_keys(edge)
        assert rc == 0 and (keys[1] == wc.derive_row(edge[1])).all(), kind2


def test_combine_by_key_set(keyset):
    keys, sk = keyset
    kc, where = kcs.host_mix(keys, sk)
    x = wc.WireCase(kc.case)
    z, _, R, S, m, offs = decoded(x)
    rc, status, got = kl.combine(keys, kc.key_idx, z, R, S, m, offs)
    assert rc == 0 and status.tolist() == kcs.KEY_STATUS
    assert mc.check(kc.case, kcs.expected(kc), got, "wire key set") == 0
    # an undecodable R: status 3 for its transcript only
    kc2 = kcs.pool_transcripts([2, 3, 1], 920, keys, sk)
    y = wc.WireCase(kc2.case)
    y.plant(1, 0, "R", "0xFF")                    # the transcript's first share: its status is the transcript's
    y.check_derived()
    z, _, R, S, m, offs = decoded(y, lanes=5)
    rc, _, got = kl.combine(keys, kc2.key_idx, z, R, S, m, offs)
    rc2, _, want = kl.combine(keys, kc2.key_idx, *[y.derived.dirty[k] for k in ("z", "R", "S", "m")], offs)
    assert rc == 0 and rc2 == 0 and all((a == b).all() for a, b in zip(got, want))
    assert got[4].tolist() == [0, 3, 0] and got[0][y.derived.row(1, 0)] == 3 and not got[2][1].any()


def verifier_inputs(c, lanes=3):
    """The case's keys and signatures as wire bytes, through the lane body: (PK, R) decoded, sig_w."""
    pk_w, sig_w = wc.compress_column(c.PK_clean), wc.sig_rows(c.u, wc.compress_column(c.R))
    return pk_w, sig_w


def test_aggregate_and_verify(keyset):
    keys, sk = keyset
    rng = np.random.default_rng(77)
    c = vc.build([vc.draw(rng, n) for n in (1, 2, 5, 3, 0, 4, 2, 3)], 1500, keys, sk)
    c.spoil_u(2)
    pk_w, sig_w = verifier_inputs(c)
    pk_w[c.row(3, 1)] = np.frombuffer(wc.encoding("v=q-1 signed"), np.uint8)       # an undecodable key: the vector is refused
    c.refused[3] = "undecodable key"
    sig_w[5, 32:] = np.frombuffer(wc.encoding("non-residue"), np.uint8)            # an undecodable R: status 3, the aggregate stays
    sig_w[6, 32:] = np.frombuffer(wc.encoding("order 2"), np.uint8)               # decodable, of order 2: InvalidPoint by the single-scheme verification
    pk, r = wh.decode([(pk_w, 0)], lanes=3)[0], wh.decode([(sig_w, 32)], lanes=3)[0]
    assert (r == wc.derive_column(sig_w[:, 32:])).all() and (r[5] == 0xFF).all() and (pk[c.row(3, 1)] == 0xFF).all()
    want = vc.expected(c, derived_R=r)
    agg, vst = vl.run(pk, c.offs32(), None)
    st, tally, agg2 = vl.run(pk, c.offs32(), (c.u, r, c.m))
    assert (agg == want[0]).all() and (vst == want[1]).all() and (agg2 == want[0]).all()
    assert (st == want[2]).all() and tally.tolist() == want[3].tolist() and int(tally.sum()) == c.B
    assert st.tolist() == [0, 0, 2, 3, 1, 3, 1, 0] and agg2[5].any() and not agg2[3].any()
    # by key set: the signature column alone is wire
    st2, tally2, agg3 = vl.run(c.key_idx, c.offs32(), (c.u, r, c.m), keys=keys)
    assert st2.tolist()[:3] == [0, 0, 2] and st2[5] == 3 and st2[6] == 1 and int(tally2.sum()) == c.B


def test_the_reference_known_answer_from_its_wire_bytes():
    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")) as f:
        k = json.load(f)["multisig_kat"]
    col = lambda xs: np.frombuffer(b"".join(bytes.fromhex(x) for x in xs), np.uint8).reshape(len(xs), 32)  # noqa: E731
    pk_w, r_w, s_w, z = col(k["public_keys"]), col(k["r_points"]), col(k["s_points"]), col(k["individual_shares"])
    m = np.frombuffer(o.le32(k["message"]), np.uint8).reshape(1, 32)
    offs = np.array([0, 3], np.uint32)
    pk, r, s = wh.decode([(pk_w, 0), (r_w, 0), (s_w, 0)], lanes=2)
    st, agg, su, sr, ts = hl.multisig(z, pk, r, s, m, offs)
    assert st.tolist() == [0, 0, 0] and ts.tolist() == [0]
    assert wc.compress_column(agg)[0].tobytes().hex() == k["aggregate_public_key"]
    assert (su[0].tobytes() + wc.compress_column(sr)[0].tobytes()).hex() == k["signature"]
    # the verifier's half from PublicKey::to_bytes and Signature::to_bytes
    sig_w = np.frombuffer(bytes.fromhex(k["signature"]), np.uint8).reshape(1, 64).copy()
    rr = wh.decode([(sig_w, 32)])[0]
    status, tally, agg2 = vl.run(pk, offs, (sig_w[:, :32], rr, m))
    assert status.tolist() == [0] and tally.tolist() == [1, 0, 0, 0] and (agg2 == agg).all()
    sig_w[0, 0] ^= 1
    status, tally, _ = vl.run(pk, offs, (sig_w[:, :32], rr, m))
    assert status.tolist() == [2] and tally.tolist() == [0, 0, 1, 0]

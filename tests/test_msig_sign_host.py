"""The signer's multisignature passes (csrc/msig_sign.h) compiled for the CPU: the map, the check pass, the front passes of the
combine call, ms_final_item and the share pass, and sign_round_1 -- against the reference's KAT bytes, against the Python
model of msig_sign_cases (sign_round_2 written out over oracle/jjs_oracle.py), and, for the shares of valid transcripts, through
the CPU build of the combine passes, which must accept every one of them."""
import json
import os

import numpy as np
import pytest

import hostlib
import jjs_oracle as o
import msig_ext_hostlib as xl
import msig_sign_cases as sc
import msig_sign_hostlib as sl
import multisig_cases as mc
from helpers import to_pt

H = bytes.fromhex


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")) as f:
        return json.load(f)["multisig_kat"]


@pytest.fixture(scope="module")
def rules():
    base, cases = sc.rule_cases()
    base_z, base_st = sc.model(base, *base.call(list(range(base.n))))
    assert not base_st.any()
    return base, base_z, cases


def written(z, st):
    assert not (z == 0xA5).all(1).any() and not (st == 0xA5).any(), "an output row was not written"


def test_reference_kat(kat):
    c = sc.kat_case(kat)
    want = np.stack([np.frombuffer(H(x), np.uint8) for x in kat["individual_shares"]])
    z, st = sl.sign(c, *c.call())
    assert st.tolist() == [0, 0, 0] and (z == want).all(), "signer_row NULL"
    z, st = sl.sign(c, *c.call([2, 0]))
    assert st.tolist() == [0, 0] and (z == want[[2, 0]]).all(), "signer_row [2, 0]"
    sc.check((z, st), sc.model(c, *c.call([2, 0])), "the model on the KAT")
    R, S, bad = sl.round1(c.r, c.s)
    assert not bad.any()
    assert [o.compress(to_pt(x)).hex() for x in R] == kat["r_points"] and [o.compress(to_pt(x)).hex() for x in S] == kat["s_points"]
    assert (R == c.R).all() and (S == c.S).all()


def test_round1_edges():
    ks = [0, 1, o.R_ORDER - 1, 2, o.R_ORDER, 5, 7, mc.ALL_ONES]
    r, s = mc._fe(ks), mc._fe(ks[::-1])
    R, S, bad = sl.round1(r, s)
    want_bad = [int(a >= o.R_ORDER or b >= o.R_ORDER) for a, b in zip(ks, ks[::-1])]
    assert bad.tolist() == want_bad and sum(want_bad) == 4
    for i, (a, b) in enumerate(zip(ks, ks[::-1])):
        if want_bad[i]:
            assert not R[i].any() and not S[i].any(), i
        else:
            assert to_pt(R[i]) == o.mul(o.G, a) and to_pt(S[i]) == o.mul(o.G, b), i


@pytest.mark.parametrize("fmt", ("affine", "ext"))
def test_ragged_call(fmt):
    c = sc.ragged()
    assert c.offsets.tolist() == [0, 1, 3, 3, 6, 14]
    x = c.to_ext(77) if fmt == "ext" else c
    if fmt == "ext":
        assert (x.PK[:, 64:] != np.frombuffer(o.le32(1), np.uint8)).any(1).all(), "Z != 1"
    z, st = sl.sign(x, *x.call())
    written(z, st)
    sc.check((z, st), sc.model(x, *x.call()), fmt)
    assert not st.any()
    rows = [13, 0, 4, 2, 2]
    got = sl.sign(x, *x.call(rows))
    written(*got)
    sc.check(got, sc.model(x, *x.call(rows)), fmt + ", signer_row given")
    assert (got[0] == z[rows]).all()
    # the shares through the existing combine item functions
    if fmt == "ext":
        share_st, _, su, _, ts = xl.combine(*sc.combine_args(x, z))
    else:
        share_st, _, su, _, ts = hostlib.multisig(*sc.combine_args(x, z))
    assert not share_st.any() and ts.tolist() == [0, 0, 5, 0, 0]
    for t in (0, 1, 3, 4):
        assert (su[t] == sc.sum_mod_r(z[c.rows_of(t)])).all(), t


def test_every_rule(rules):
    base, base_z, cases = rules
    assert len(cases) == 17
    for rule in cases:
        got = sl.sign(rule.case, rule.signer_row, rule.sk, rule.r, rule.s)
        written(*got)
        sc.check_rule(rule, base_z, got)
        sc.check(got, sc.model(rule.case, rule.signer_row, rule.sk, rule.r, rule.s), rule.name)


def test_duplicates_across_transcripts():
    c = sc.across_transcripts()
    assert (c.R[0] == c.R[3]).all()
    got = sl.sign(c, *c.call())
    assert not got[1].any() and got[0].any(1).all()
    sc.check(got, sc.model(c, *c.call()))


def test_all_transcripts_empty():
    c = sc.build([0, 0], 3)
    rows, sk, r, s = np.array([0, sc.NO_ROW], np.uint32), mc._fe([1, 2]), mc._fe([3, 4]), mc._fe([5, 6])
    z, st = sl.sign(c, rows, sk, r, s)
    assert st.tolist() == [3, 3] and not z.any()


def test_257_participants():
    """One past the generated tag table: the shares against the model's recorded ones (msig_sign_cases.recorded_257) and through
    the CPU build of the combine passes; then S duplicated at rows 0 and 256, the two ends of the scan."""
    c = sc.long_case()
    z, st = sl.sign(c, *c.call())
    sc.check((z, st), sc.model(c, *c.call(), recorded=sc.recorded_257(c)), "257")
    assert not st.any()
    share_st, _, su, _, ts = hostlib.multisig(*sc.combine_args(c, z))
    assert not share_st.any() and ts.tolist() == [0] and (su[0] == sc.sum_mod_r(z)).all()
    d = c.copy()
    d.S[256] = d.S[0]; d.s[256] = d.s[0]
    z, st = sl.sign(d, *d.call())
    assert st.tolist() == [7] * 257 and not z.any()

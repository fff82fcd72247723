"""verify_share on its own (csrc/msig_share.h) compiled for the CPU: the stage functions of the three routes, one item after the
other in the device's launch order, on the cases of msig_share_cases in the three input formats.  Expected statuses are the C
oracle's share_status with the query's z at its row (and the Python oracle's multisig_verify_share for transcripts of up to
three participants), expected sig_R the oracles' RSa, the statuses 3 and 5 written out from the rules of include/jjs_gpu.h."""
import numpy as np
import pytest

import msig_share_cases as shc
import msig_share_hostlib as hl


@pytest.fixture(scope="module")
def inline():
    sc = shc.inline_case()
    return sc, shc.expected_status(sc), shc.expected_R(sc)


@pytest.fixture(scope="module")
def groups():
    return [(name, sc, shc.expected_status(sc), shc.expected_R(sc)) for name, sc in shc.group_cases()]


@pytest.fixture(scope="module")
def keyset():
    sc = shc.keyset_case()
    return sc, shc.expected_status(sc), shc.expected_R(sc)


def written(st, sr):
    assert not (st == 0xA5).any(), "a status was not written"
    assert sr is None or not (sr == 0xA5).all(1).any(), "a row of sig_R was not written"


def test_the_cases_hold_what_they_should(inline, groups, keyset):
    sc, want, want_R = inline
    assert {0, 3, 4, 5} <= set(want.tolist())
    assert sc.case.sizes()[:5].tolist() == [1, 2, 3, 0, 8] and 5 not in sc.qt
    by_t = lambda t: [int(w) for w, qt in zip(want, sc.qt) if qt == t]  # noqa: E731
    for t in (6, 8, 10):                                   # R coordinate, m, PK coordinate: every query 3, the neighbours not
        assert set(by_t(t)) == {3} and not want_R[t].any(), t
        near = by_t(t - 1) + by_t(t + 1)                   # (5 has no query; 11 also has the two queries beyond its last slot)
        assert 3 not in near and 4 not in near and near.count(0) >= 2, t
    assert not want_R[3].any() and want_R[5].any()
    # the Python oracle on the transcripts of up to three participants
    plan = shc.plan(sc)
    small = [q for q in range(sc.Q) if plan[q] < 0 and sc.case.sizes()[sc.qt[q]] <= 3]
    assert len(small) > 20
    for q in small:
        assert shc.python_oracle_status(sc, q) == want[q], sc.what[q]
    # the torsion key's shares are valid ones (the reference accepts them), under every other small-order key the oracle decides
    name, tsc, twant, _ = groups[-1]
    assert name == "torsion key" and not twant[:tsc.case.n].any()
    ksc, kwant, kR = keyset
    assert len(ksc.refused) == 5 and all(not kR[t].any() for t in ksc.refused)


@pytest.mark.parametrize("fmt", shc.FORMATS)
def test_inline(inline, fmt):
    sc, want, want_R = inline
    st, sr = hl.verify_share(sc, fmt)
    written(st, sr)
    shc.check(sc, want, want_R, st, sr, fmt)
    st2, none = hl.verify_share(sc, fmt, want_R=False, lanes=1)
    assert none is None and (st2 == st).all()


@pytest.mark.parametrize("fmt", shc.FORMATS)
def test_groups(groups, fmt):
    for name, sc, want, want_R in groups:
        st, sr = hl.verify_share(sc, fmt)
        written(st, sr)
        shc.check(sc, want, want_R, st, sr, f"{name}, {fmt}")
        if fmt == "affine":                                  # the same transcripts through the inline route
            ist, isr = hl.verify_share(shc.as_route(sc, "inline"), fmt)
            assert (ist == st).all() and (isr == sr).all(), name


@pytest.mark.parametrize("fmt", shc.FORMATS)
def test_keyset(keyset, fmt):
    sc, want, want_R = keyset
    st, sr = hl.verify_share(sc, fmt)
    written(st, sr)
    shc.check(sc, want, want_R, st, sr, fmt)
    if fmt == "affine":                                      # the usable transcripts through the inline route on the gathered keys
        ist, isr = hl.verify_share(shc.as_route(sc, "inline"), fmt)
        ok_q = np.array([t >= sc.T or t not in sc.refused for t in sc.qt])
        ok_t = np.array([t not in sc.refused for t in range(sc.T)])
        assert (ist[ok_q] == st[ok_q]).all() and (isr[ok_t] == sr[ok_t]).all()


def test_no_queries_still_fills_sig_R(inline):
    sc, _, want_R = inline
    x = shc.ShareCase("inline", sc.case)
    st, sr = hl.verify_share(x)
    assert st.shape == (0,) and (sr == want_R).all()

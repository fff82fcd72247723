"""The verifier's multisignature passes (csrc/msig_verify.h) compiled for the CPU: the map, the check (or the key set's gather),
the delinearisation and the sum, then the CPU build's single-scheme verification on the aggregate column and the clear pass --
the standard mix of msig_verify_cases in inline and key-set form and in affine and extended format, against the oracle
(jjs_oracle_c.multisig_combine for the aggregates, jjs_oracle_c.verify_single for the statuses), against the CPU build of the
inline combine passes (hostlib.multisig's agg_pk, byte for byte on the usable non-empty vectors), with every output prefilled
and every row written; and the two edge calls, every vector refused and every vector empty."""
import numpy as np
import pytest

import hostlib
import msig_keyset_cases as kcs
import msig_verify_cases as vc
import msig_verify_hostlib as vl

FORMS = ("inline", "keyset")


@pytest.fixture(scope="module")
def keyset():
    return kcs.key_set()


def written(*outs):
    for x in outs:
        assert x.size == 0 or not (x.reshape(len(x), -1) == 0xA5).all(1).any(), "an output row was not written"


def both_calls(c, form, keys, ext=None):
    """The aggregation call and the verification call of a case; returns (agg, vst), (st, tally, agg)."""
    rows = c.PK if form == "inline" else c.key_idx
    R = c.R
    if ext is not None:
        rows, R = (ext.PK if form == "inline" else c.key_idx), ext.R
    kw = dict(keys=keys if form == "keyset" else None)
    a = vl.run(rows, c.offs32(), None, ext=ext is not None and form == "inline", **kw)
    v = vl.run(rows, c.offs32(), (c.u, R, c.m), ext=ext is not None, **kw)
    written(*a); written(v[0], v[2])
    return a, v


def check(c, a, v, want, label):
    agg, vst, st, tally = want
    assert (a[0] == agg).all() and (a[1] == vst).all(), (label, "aggregation", np.nonzero((a[0] != agg).any(1))[0][:8].tolist())
    assert (v[2] == agg).all(), (label, "agg_pk of the verification", np.nonzero((v[2] != agg).any(1))[0][:8].tolist())
    assert (v[0] == st).all(), (label, "status", np.nonzero(v[0] != st)[0][:8].tolist(), v[0][v[0] != st][:8].tolist(), st[v[0] != st][:8].tolist())
    assert v[1].tolist() == tally.tolist(), (label, "tally")


def against_inline_passes(c, agg, label):
    """agg_pk of the CPU build's combine passes on the same keys with dummy shares, for the usable non-empty vectors."""
    ident = np.tile(vc.IDENT, (c.n, 1))
    ref = hostlib.multisig(np.zeros((c.n, 32), np.uint8), c.PK_clean, ident, ident, np.zeros((c.B, 32), np.uint8), c.offs32())[1]
    mask = c.usable() & (c.sizes() > 0)
    assert mask.sum() > c.B // 2 and (agg[mask] == ref[mask]).all(), label


@pytest.mark.parametrize("form", FORMS)
def test_standard_mix_affine(keyset, form):
    keys, sk = keyset
    c = vc.standard_mix(keys, sk, form)
    assert 90 <= c.B <= 110 and 300 <= c.n <= 450
    a, v = both_calls(c, form, keys)
    check(c, a, v, vc.expected(c), form)
    vc.check_named(c, form, v[2], v[0], form)
    against_inline_passes(c, a[0], form)
    causes = vc.INLINE_REFUSALS if form == "inline" else tuple(w for w, _ in vc.KEYSET_REFUSALS)
    assert sorted(c.refused.values()) == sorted(causes)
    print(form, "statuses", v[0].tolist(), "tally", v[1].tolist())


@pytest.mark.parametrize("form", FORMS)
def test_standard_mix_extended(keyset, form):
    keys, sk = keyset
    x = vc.ext_mix(keys, sk, form)
    c = x.case
    a, v = both_calls(c, form, keys, ext=x)
    check(c, a, v, vc.expected(c, derived_R=x.derived_R), form + " ext")
    vc.check_named(c, form, v[2], v[0], form + " ext")
    against_inline_passes(c, a[0], form + " ext")
    assert v[0][c.where["R Z=0"]] == 3 and v[2][c.where["R Z=0"]].any()
    if form == "inline":
        t = c.where["key Z=0"]
        assert v[0][t] == 3 and a[1][t] == 3 and not v[2][t].any()
        assert (np.asarray(x.PK)[:, 64:] != np.eye(1, 32, dtype=np.uint8)).any(1).sum() > c.n // 2, "Z != 1 rows"


@pytest.mark.parametrize("form", FORMS)
def test_every_vector_refused_and_every_vector_empty(keyset, form):
    keys, sk = keyset
    c = vc.build([[0, 1], [2], [3, 4, 5]], 1400, keys, sk)
    for t in range(3):
        if form == "inline":
            c.refuse_inline(t, 0, vc.INLINE_REFUSALS[t])
        else:
            c.refuse_keyset(t, 0, *vc.KEYSET_REFUSALS[t][::-1])
    a, v = both_calls(c, form, keys)
    check(c, a, v, vc.expected(c), form + " all refused")
    assert not a[0].any() and (a[1] == 3).all() and (v[0] == 3).all() and not v[2].any() and v[1].tolist() == [0, 0, 0, 3]
    c = vc.build([[], []], 1401, keys, sk)
    a, v = both_calls(c, form, keys)
    check(c, a, v, vc.expected(c), form + " all empty")
    assert (a[0] == vc.IDENT).all() and (a[1] == 0).all() and (v[0] == 1).all() and v[1].tolist() == [0, 2, 0, 0]

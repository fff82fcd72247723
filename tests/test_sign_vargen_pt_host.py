"""csrc/sign_vargen.h on the CPU build against the oracle: every case of sign_vargen_pt_cases.py in all three formats, the
per-item body and the shared-generator body (its tables built by the CPU build of the table functions), the derivation, and the
reference's own bytes.  Every comparison is byte for byte.  No GPU."""
import numpy as np
import pytest

import jjs_oracle as o
import sign_vargen_hostlib as hl
import sign_vargen_pt_cases as vc
from helpers import to_int, to_pt


@pytest.mark.parametrize("fmt", vc.FORMATS)
def test_every_case_signs_as_the_oracle(fmt):
    c = vc.call(fmt)
    assert sorted(np.nonzero(c.status)[0].tolist()) == sorted((vc.FIRST_PLACES + vc.MORE_PLACES)[:len(vc.KINDS[fmt])])
    for lanes in (1, 5):
        got = hl.sign(vc.FORMAT_CODE[fmt], c.sk, c.Gen, c.rnd, c.m, lanes=lanes)
        vc.check(got, c, (fmt, lanes))
    u, R, PK, G_out, st = hl.sign(vc.FORMAT_CODE[fmt], c.sk, c.Gen, c.rnd, c.m, want_pk=False, want_gen=False)
    assert PK is None and G_out is None and (u == c.u).all() and (R == c.R).all() and st.tolist() == c.status.tolist()


@pytest.mark.parametrize("fmt", vc.FORMATS)
def test_every_case_derives_as_the_oracle(fmt):
    c = vc.call(fmt)
    # the derivation knows no rnd and no m: those two malformed rows are good rows to it
    PK, G_out, st = hl.derive(vc.FORMAT_CODE[fmt], c.sk, c.Gen)
    for i in range(c.n):
        if c.status[i] == 0:
            assert st[i] == 0 and (PK[i] == c.PK[i]).all() and (G_out[i] == c.Gen_out[i]).all(), (fmt, c.labels[i])
        elif "rnd=r" in c.labels[i] or "m=q" in c.labels[i]:
            assert st[i] == 0 and to_pt(PK[i]) == o.mul(to_pt(G_out[i]), to_int(c.sk[i])) and o.is_on_curve(to_pt(G_out[i])), (fmt, c.labels[i])
        else:
            assert st[i] == 3 and not PK[i].any() and not G_out[i].any(), (fmt, c.labels[i])


def test_the_oracle_refuses_what_the_cases_expect_it_to():
    c = vc.call("affine")
    by_gen = vc.expected_verify_by_generator()
    seen = set()
    for i in range(c.n):
        if c.status[i]:
            continue
        label = c.labels[i].split(" sk=")[0]
        want = 1 if to_int(c.sk[i]) == 0 else by_gen[label]          # sk = 0: the key is the identity
        assert c.verify[i] == want, c.labels[i]
        seen.add((label, want))
    assert {w for _, w in seen} == {0, 1}
    assert by_gen["identity"] == by_gen["order 4"] == by_gen["P+3T"] == 1 and by_gen["P+0T"] == by_gen["5*G"] == 0


@pytest.mark.parametrize("fmt", vc.FORMATS)
@pytest.mark.parametrize("which", vc.SHARED_GENERATORS + ("order 8", "unusable"))
def test_one_generator_for_the_call_both_bodies(which, fmt):
    n = 5
    sk, Gen, rnd, m, p = vc.shared_call(which, n, fmt)
    per_item = hl.sign(vc.FORMAT_CODE[fmt], sk, Gen, rnd, m, route=0)
    tabled = hl.sign(vc.FORMAT_CODE[fmt], sk, Gen, rnd, m, route=1)
    tiled = hl.sign(vc.FORMAT_CODE[fmt], sk, np.tile(Gen, (n, 1)), rnd, m, route=0)
    for a, b in zip(per_item, tabled):
        assert (a == b).all(), (which, fmt, "the two routes")
    for k in (0, 1, 2, 4):
        assert (per_item[k] == tiled[k]).all(), (which, fmt, "against the per-item call with the generator tiled")
    u, R, PK, G_out, st = per_item
    assert G_out.shape == (1, 64)
    if which == "unusable":
        assert st.tolist() == [3] * n and not (u.any() or R.any() or PK.any() or G_out.any())
        return
    assert st.tolist() == [0] * n and to_pt(G_out[0]) == p and (tiled[3] == G_out[0]).all()
    for i, (wu, wR, wPK) in vc.oracle_rows(sk, p, rnd, m, range(n)).items():
        assert (u[i] == wu).all() and (R[i] == wR).all() and (PK[i] == wPK).all(), (which, fmt, i)


def test_one_item_with_one_generator_is_the_per_item_call():
    sk, Gen, rnd, m, p = vc.shared_call("5*G", 1)
    sk[0] = np.frombuffer(o.le32(o.R_ORDER), np.uint8)
    for route in (0, 1):
        u, R, PK, G_out, st = hl.sign(0, sk, Gen, rnd, m, route=route)
        assert st.tolist() == [3] and not (u.any() or R.any() or PK.any() or G_out.any()), "the item's generator row is zero with it"
    sk2, _, rnd2, m2, _ = vc.shared_call("5*G", 2)
    sk2[0] = sk[0]
    u, R, PK, G_out, st = hl.sign(0, sk2, Gen, rnd2, m2)
    assert st.tolist() == [3, 0] and to_pt(G_out[0]) == p, "a shared generator's row does not depend on item 0"


def test_the_references_own_bytes(reference_kat):
    k = vc.kat(reference_kat)
    sk = np.frombuffer(k["secret"][:32], np.uint8).reshape(1, 32)
    gen_w = np.frombuffer(k["secret"][32:], np.uint8).reshape(1, 32)
    PK, G_out, st = hl.derive(2, sk, gen_w)
    assert st.tolist() == [0]
    assert o.compress(to_pt(PK[0])) + o.compress(to_pt(G_out[0])) == k["public"]
    for route in (0, 1):
        u, R, PK2, _, st = hl.sign(2, sk, gen_w, k["rnd"].reshape(1, 32), k["m"].reshape(1, 32), route=route)
        assert st.tolist() == [0] and (PK2 == PK).all()
        assert u[0].tobytes() + o.compress(to_pt(R[0])) == k["signature"]

"""csrc/sign_fixed.h on the CPU build against the oracle: every row of sign_fixed_cases.py in both schemes, the per-item body and
the pre-pass with the keyed body, affine and wire outputs, the derivation, and the reference's own bytes.  Every comparison is
byte for byte.  No GPU."""
import numpy as np
import pytest

import jjs_oracle as o
import sign_fixed_cases as fc
import sign_fixed_hostlib as hl
from helpers import fe_bytes, to_int

SCHEMES = (False, True)


@pytest.mark.parametrize("double", SCHEMES)
def test_every_case_signs_as_the_oracle(double):
    c = fc.call(double)
    assert sorted(np.nonzero(c.status)[0].tolist()) == sorted(fc.PLACES)
    fc.check(hl.sign(double, c.sk, c.rnd, c.m), c, double)
    for name in fc.outputs_of(double):                   # each output NULL in turn: the others do not change
        got = hl.sign(double, c.sk, c.rnd, c.m, skip=(name,))
        assert got[name] is None
        fc.check(got, c, (double, "without", name), skip=(name,))
    wire_only = hl.sign(double, c.sk, c.rnd, c.m, skip=("u", "R", "Rp", "PK", "PKp"))
    fc.check(wire_only, c, (double, "wire alone"), skip=("u", "R", "Rp", "PK", "PKp"))


@pytest.mark.parametrize("double", SCHEMES)
def test_the_oracle_verifies_what_the_cases_expect_it_to(double):
    c = fc.call(double)
    for i in range(c.n):
        if c.status[i] == 0:
            assert c.verify[i] == (1 if to_int(c.sk[i]) == 0 else 0), c.labels[i]      # sk = 0: the key is the identity, InvalidPoint
    assert sorted(c.verify[c.status == 0].tolist())[-1] == 1


@pytest.mark.parametrize("double", SCHEMES)
def test_every_case_derives_as_the_oracle(double):
    c = fc.call(double)
    got = hl.derive(double, c.sk)
    for i in range(c.n):
        sk = to_int(c.sk[i])
        if sk >= o.R_ORDER:
            assert got["status"][i] == 3 and not any(got[k][i].any() for k in fc.key_rows(double, 0)), c.labels[i]
            continue
        # the derivation knows no rnd and no m: those malformed rows are good rows to it
        assert got["status"][i] == 0, c.labels[i]
        for k, want in fc.key_rows(double, sk).items():
            assert (got[k][i] == want).all(), (k, c.labels[i])
    only_wire = hl.derive(double, c.sk, skip=("PK", "PKp"))
    assert (only_wire["pk_w"] == got["pk_w"]).all() and only_wire["PK"] is None


@pytest.mark.parametrize("double", SCHEMES)
@pytest.mark.parametrize("which", fc.KEYED_KEYS)
@pytest.mark.parametrize("n", (1, 2, 64))
def test_one_key_for_the_call_both_bodies(which, double, n):
    sk, rnd, m = fc.keyed_call(double, which, n)
    per_item = hl.sign(double, sk, rnd, m, route=0)
    keyed = hl.sign(double, sk, rnd, m, route=1)
    tiled = hl.sign(double, np.tile(sk, (n, 1)), rnd, m, route=0)
    names = fc.outputs_of(double)
    for k in names + ("status",):
        assert (per_item[k] == keyed[k]).all(), (which, double, n, k, "the two routes")
    for k in ("u", "R", "Rp", "sig_w", "status"):
        if per_item[k] is not None:
            assert (per_item[k] == tiled[k]).all(), (which, double, n, k, "against the per-item call with the key tiled")
    key_names = [k for k in names if k in ("PK", "PKp", "pk_w")]
    assert all(per_item[k].shape[0] == 1 for k in key_names)
    if which == "unusable":
        assert per_item["status"].tolist() == [3] * n and not any(per_item[k].any() for k in names)
        return
    bad_first = n > 2                                    # keyed_call: row 0 has rnd = r
    assert per_item["status"].tolist() == ([3] if bad_first else [0]) + [0] * (n - 1)
    for k, want in fc.key_rows(double, fc.keyed_key(which)).items():
        assert (per_item[k][0] == want).all(), (which, double, n, k, "the key rows are the key's whatever item 0 is")
        assert (tiled[k][n - 1] == want).all()
    if bad_first:
        assert not any(per_item[k][0].any() for k in names if k not in key_names) and not any(tiled[k][0].any() for k in names)
    rows = [i for i in (0, 1, n // 2, n - 1) if i < n and not (bad_first and i == 0)]
    for i, want in fc.oracle_rows(double, sk, rnd, m, rows).items():
        for k in names:
            if k not in key_names:
                assert (per_item[k][i] == want[k]).all(), (which, double, n, k, i)


@pytest.mark.parametrize("double", SCHEMES)
def test_one_item_with_one_key_is_the_per_item_call(double):
    sk, rnd, m = fc.keyed_call(double, "random", 1)
    rnd[0] = fe_bytes(o.R_ORDER)
    for route in (0, 1):
        got = hl.sign(double, sk, rnd, m, route=route)
        assert got["status"].tolist() == [3] and not any(got[k].any() for k in fc.outputs_of(double)), "the item's key row is zero with it"


def test_the_references_own_bytes(reference_kat):
    k = fc.kat(reference_kat)
    assert k["secret"] == k["sk"].tobytes()
    sk = k["sk"].reshape(1, 32)
    assert hl.derive(False, sk)["pk_w"][0].tobytes() == k["public"]
    assert hl.derive(True, sk)["pk_w"][0].tobytes() == k["public_double"]
    pairs = np.stack([s for s, _ in k["pairs"]])
    got = hl.derive(False, pairs)
    assert got["status"].tolist() == [0, 0, 0] and [r.tobytes() for r in got["pk_w"]] == [p for _, p in k["pairs"]]
    for route in (0, 1):
        s = hl.sign(False, sk, k["rnd"].reshape(1, 32), k["m"].reshape(1, 32), route=route)
        assert s["status"].tolist() == [0] and s["sig_w"][0].tobytes() == k["signature"] and s["pk_w"][0].tobytes() == k["public"]
        d = hl.sign(True, sk, k["rnd_double"].reshape(1, 32), k["m"].reshape(1, 32), route=route)
        assert d["status"].tolist() == [0] and d["sig_w"][0].tobytes() == k["signature_double"] and d["pk_w"][0].tobytes() == k["public_double"]

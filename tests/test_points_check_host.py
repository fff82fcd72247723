"""`is_valid` alone on the CPU build: the per-point functions of csrc/points_check.h -- the code of the device's lanes -- over
the case lists of points_check_cases.py, against oracle.point_is_valid, oracle.decompress and Python integers: every status, the
tally and every output row, the zeroed ones included.  No GPU."""
import numpy as np
import pytest

import jjs_oracle as o
import points_check_cases as pc
import points_check_hostlib as hl


def _outputs(kind, scheme):
    if kind == "keys":
        return [True, scheme != "single"]
    return [True, True, scheme == "double"]


@pytest.mark.parametrize("kind,scheme,fmt", pc.ALL)
def test_statuses_tally_and_outputs(kind, scheme, fmt):
    case = pc.build(kind, scheme, fmt)
    have = _outputs(kind, scheme)
    for want_outs in ([False] * len(have), have):
        st, tally, outs = hl.check(kind, pc.SCHEMES[scheme], pc.FORMATS[fmt], case["cols"], want_outs)
        bad = np.where(st != case["status"])[0]
        assert len(bad) == 0, (bad[:8], st[bad[:8]], case["status"][bad[:8]])
        assert tally.tolist() == case["tally"].tolist() and tally[2] == 0
        for j, (got, want) in enumerate(zip(outs, case["outs"])):
            if got is None:
                continue
            rows = np.where((got != want).any(1))[0]
            assert len(rows) == 0, (j, rows[:8], case["status"][rows[:8]])


@pytest.mark.parametrize("want_outs", [[True, False], [False, True]])
def test_one_of_two_outputs_of_extended_keys(want_outs):
    """the normaliser writes the column nobody asked for somewhere else; the other is as in the call with both"""
    case = pc.build("keys", "double", "ext")
    st, tally, outs = hl.check("keys", 1, 1, case["cols"], want_outs)
    assert (st == case["status"]).all() and tally.tolist() == case["tally"].tolist()
    for got, want in zip(outs, case["outs"]):
        assert got is None or (got == want).all()


@pytest.mark.parametrize("fmt", list(pc.FORMATS))
def test_every_point_by_its_own_function(fmt):
    """every point case through pc_affine_point / pc_ext_point / pc_wire_point alone: none is skipped"""
    seen = {0: 0, 1: 0, 3: 0}
    for row, want, out in pc.point_cases(fmt):
        st, dec = hl.point(fmt, row)
        assert st == want, (fmt, row.tobytes().hex(), st, want)
        if dec is not None and want != 3:
            assert (dec == out).all()
        seen[want] += 1
    assert all(v >= 8 for v in seen.values()), seen


def test_the_projective_tests_are_the_affine_ones_scaled():
    """(U : V : Z) and (cU : cV : cZ) get one status, and that of (U/Z, V/Z): restated with Python integers"""
    rng = np.random.default_rng(3)
    for row, want, _ in pc.point_cases("affine"):
        if want == 3:
            continue
        u, v = pc.to_pt(row)
        for _ in range(2):
            z = int.from_bytes(rng.bytes(40), "little") % (o.Q - 1) + 1
            ext = np.concatenate([pc.fe_bytes(u * z % o.Q), pc.fe_bytes(v * z % o.Q), pc.fe_bytes(z)])
            assert hl.point("ext", ext)[0] == want


def test_empty_call():
    st, tally, outs = hl.check("keys", 0, 0, [np.zeros((0, 64), np.uint8), None], [True, False])
    assert len(st) == 0 and tally.tolist() == [0, 0, 0, 0]

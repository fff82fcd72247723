"""The cases and the Python reference of tests/msm_cases.py against the CPU build, before the device sees them: the bucket
MSM of csrc/msm.h (tests/hostbuild/host_msm.h runs its steps in loops) for every window width from 8 to 16 in both shapes --
the buckets' offsets, the sorted entries bucket by bucket as sets, every window sum and the total -- and the run sums and key
points of csrc/keyset_verdict.h under chosen scalar columns.  Every comparison is an equality of integers or of points.  No
GPU."""
import numpy as np
import pytest

import keyset_verdict_hostlib as kvh
import msm_cases as mc
import verdict_hostlib as vh
from helpers import to_pt


def point_eq_affine(got, want, what):
    assert to_pt(got) == want, what


@pytest.mark.parametrize("c,short", mc.SHAPES)
def test_msm_stages_match_the_reference(c, short):
    for g in mc.msm_groups(c, short):
        ref = mc.msm_reference(g, c, short)
        pts, sc = mc.msm_inputs(g)
        t = np.arange(len(sc))
        neg = ((g["neg_kinds"] >> (t // g["n"])) & 1).astype(np.uint8)
        got = vh.msm(pts, sc, neg, c=c, short=short, stages=True)
        mc.check_msm(ref, got["off"], got["order"], got["win"], got["total"], (c, short, g["name"]), point_eq_affine)
        if g["name"] == "scalars":
            mc.check_end_slots(c, short, ref)
            if not short:
                mc.check_top_slots(c, ref)


def test_msm_case_classes_are_all_populated():
    mc.CLASS_COUNTS.clear()
    for c, short in mc.SHAPES:
        mc.msm_groups(c, short)
    mc.assert_msm_classes()


@pytest.mark.parametrize("scheme,nk", mc.KEYSET_SETS)
def test_keyset_run_sums_and_key_points(scheme, nk):
    _, keys = mc.keyset_keys(scheme, nk)
    cases = mc.keyset_cases(scheme, nk)
    sums, points = kvh.key_sums(scheme, keys, [case["idx"] for case in cases], [case["a"] for case in cases])
    for case, s, p in zip(cases, sums, points):
        mc.check_keyset(case, s, p, case["name"], point_eq_affine)


def test_keyset_case_classes_are_all_populated():
    mc.CLASS_COUNTS.clear()
    for scheme, nk in mc.KEYSET_SETS:
        mc.keyset_cases(scheme, nk)
    mc.assert_keyset_classes()

"""The scalar multiplications of the product's headers on the CPU build, with crafted scalars and points (tests/
scalar_mul_cases.py): recoding into signed digits, the window look-ups and their clamps, the shared doubling chains, the fixed-base
comb, the key tables of both widths and the latency path at 4, 8 and 16 positions, through the stage bodies of
tools/scalar_stages.h (the same ones tools/scalarcheck runs on the device).  Every output is compared, exactly, with the Python
oracle's big-integer curve arithmetic.  End to end these functions only ever meet scalars that are hash outputs; here they
meet the digit patterns a sender could choose.

Sensitivity, each edit alone on a scratch copy of the CPU build: see DESIGN.md section 6."""
import pytest

import hostlib as hl
import scalar_mul_cases as smc


@pytest.fixture(scope="module")
def recs():
    r = smc.build_records(device=False)
    out = hl.scalar_records(smc.input_words(r), smc.output_words(r))
    return smc.attach_outputs(r, out)


def test_case_classes_are_all_populated(recs):
    assert smc.CLASS_COUNTS and all(v > 0 for k, v in smc.CLASS_COUNTS.items() if not k.endswith("clamped")), smc.CLASS_COUNTS
    assert len(recs) == 13


def test_comb_mul(recs):
    smc.check_comb(recs)


def test_table_mul(recs):
    smc.check_table(recs)


def test_check_equation_fixed_and_per_item_generator(recs):
    smc.check_equations(recs)


def test_key_tables_both_widths(recs):
    smc.check_kt(recs)


def test_latency_path_pieces_and_tables(recs):
    smc.check_latency_path(recs)

"""Inversion, inverse square roots, point decoding and the normalisation of extended coordinates on the CPU build, with the
crafted inputs of tests/ingest_cases.py, through the stage bodies of tools/ingest_stages.h (the same ones tools/ingestcheck
runs on the device); and the square-root tables of the CPU build, every entry.  Every output word is compared with Python
integers.  End to end these functions meet pseudo-random field elements only; here they meet the values a sender could choose:
whole batches of halvings, limb patterns of both radices, every byte value of the 2-adic logarithm at every position, every
odd low byte (no root), Z = 0 under every mask and at every place of a lane.

Division steps (ingest_cases.RECORDED, held against every run): over the 2 816 inversion inputs of this module, crafted and
random, with the longest that a seeded search of 4 500 evaluations finds, an input needs between 501 and 531 steps, 514 on
average; fq_inverse does 600.  No input found comes near the 571 steps that would reach the last batch, so nothing here can
tell 20 batches from 19 (no bound on the count is asserted).

Sensitivity, each edit alone on a scratch copy of the CPU build: see DESIGN.md section 6.8."""
import numpy as np
import pytest

import hostlib as hl
import ingest_cases as ic


@pytest.fixture(scope="module")
def recs():
    r = ic.build_records()
    out = hl.ingest_records(ic.input_words(r), ic.output_words(r))
    return ic.attach_outputs(r, out)


def test_case_classes_are_all_populated(recs):
    assert ic.CLASS_COUNTS and all(v > 0 for k, v in ic.CLASS_COUNTS.items() if k != ic.NEGATIVE_D), ic.CLASS_COUNTS
    assert len(recs) == 34
    assert ic.DRAWS["drawn"] < 8192


def test_recorded_figures_are_those_of_this_run(recs):
    """the step counts and case counts that DESIGN.md 6.8 and the docstring above quote (ingest_cases.RECORDED) are what this
    run finds; no bound on the step count is set"""
    print("division steps over the inversion inputs:", ic.STEP_STATS)
    ic.check_recorded()


def test_one_batch_applied_to_d_and_e(recs):
    ic.check_update(ic.update_cases(), recs["one batch applied to d and e"]["out"].reshape(-1, 20))


def test_inverse(recs):
    ic.check_inv(ic.inversion_cases(), recs["inverse"]["out"].reshape(-1, 8))


def test_end_of_the_inversion(recs):
    ic.check_finish(ic.finish_cases(), recs["end of the inversion"]["out"].reshape(-1, 10))


def test_inverse_square_root(recs):
    ic.check_inv_sqrt(ic.inv_sqrt_cases(), recs["inverse square root"]["out"].reshape(-1, 8))


def test_decompress(recs):
    cases, want = ic.decompress_cases()
    out = recs["decompress"]["out"].reshape(-1, 20)
    assert not out[:, 17:].any()
    ic.check_decompress(cases, want, np.ascontiguousarray(out[:, :16]).view(np.uint8).reshape(-1, 64), out[:, 16])


def test_decompress_export_agrees(recs):
    """the harness's older export on the same encodings (it shares the tables of the stage)"""
    cases, want = ic.decompress_cases()
    aff, ok = hl.decompress(np.frombuffer(b"".join(e for _, e in cases), np.uint8).reshape(-1, 32))
    ic.check_decompress(cases, want, aff, ok)


def test_normalize(recs):
    n = 0
    for r in recs.values():
        if r["kind"] == "K_NORMALIZE":
            ic.check_normalize(r)
            n += 1
    assert n == len(ic.normalize_records()) == 28


def test_dlog_tables_host(recs):
    """all 7 x 256 powers and the 65 536 bytes of the CPU build's tables against Python"""
    ic.check_tables(*ic.table_dump(recs["tables"]))

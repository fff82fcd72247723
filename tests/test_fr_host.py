"""The scalar arithmetic modulo the group order r on the CPU build, with crafted inputs (tests/fr_cases.py): fr_mont_mul,
fr_mul, fr_sub_mul, fr_add, half_scalar_times_u, truncate250, chacha20_block and bv_weights through the stage bodies of
tools/fr_stages.h (the same ones tools/frcheck runs on the device).  Every output is compared, exactly, with Python integers
and with a ChaCha20 written in Python from RFC 8439, which is held against the RFC's vector first.  End to end these functions
are only seen through a verdict bit or a signer's u; here they meet the carries, masks and selects a batch rarely reaches.
Then the per-item passes that produce and consume those scalars, bv_item and ksv_item with the block sums of
verdict_item_pass, under the pinned seed (tests/verdict_item_cases.py): every scalar, partial sum, total and the fail word
against the Python ChaCha20, the oracle's challenges and Python integers.

Sensitivity, each edit alone on a scratch copy of the CPU build: see DESIGN.md section 6.10."""
import pytest

import fr_cases as frc
import hostlib as hl
import keyset_verdict_hostlib as kvh
import verdict_hostlib as vh
import verdict_item_cases as vic


@pytest.fixture(scope="module")
def recs():
    r = frc.build_records()
    out = hl.fr_records(frc.input_words(r), frc.output_words(r))
    return frc.attach_outputs(r, out)


def test_python_chacha20_matches_rfc8439():
    frc.check_chacha20_against_rfc()


def test_case_classes_are_all_populated(recs):
    frc.classes_populated()
    assert len(recs) == 9


def test_fr_mont_mul(recs):
    frc.check_mont_mul(recs)
    print("out of contract, results >= r:", frc.OUT_OF_CONTRACT_GE_R)


def test_fr_mul(recs):
    frc.check_mul(recs)


def test_fr_sub_mul(recs):
    frc.check_sub_mul(recs)


def test_fr_add(recs):
    frc.check_add(recs)


def test_half_scalar_times_u(recs):
    frc.check_half(recs)


def test_truncate250_both_representatives(recs):
    frc.check_truncate250(recs)


def test_chacha20_block(recs):
    frc.check_chacha20(recs)


def test_bv_weights_every_width_and_items_beyond_32_bits(recs):
    frc.check_weights(recs)


# ---- the per-item passes of the two verdict algorithms under the pinned seed (tests/verdict_item_cases.py) -----------------------
@pytest.mark.parametrize("scheme", vic.SCHEMES)
def test_verdict_item_pass_scalars_partial_sums_and_fail_word(scheme):
    cases, runs = vic.verdict_cases(scheme), {}
    for case in cases:
        blocks = case["blocks"] or vic.own_grid(len(case["b"]["u"]))
        want = vic.expected(scheme, case, blocks)
        grids = tuple(vic.grids_of(cases, case))
        key = (case["b"]["u"].tobytes(), case["b"]["R"].tobytes(), case["b"]["PK"].tobytes(), case["c"], grids)
        if key not in runs:                                   # one run of the CPU build per (batch, width): every grid's partial sums
            runs[key] = vh.verdict_items(scheme, vic.batch_columns(scheme, case["b"]), frc.PINNED_SEED, case["c"], grids)
        vic.compare((scheme, case["name"]), want, runs[key], blocks)
    assert len(runs) <= len(cases) - len(vic.FORCED_BLOCKS)
    vic.classes_populated(keysets=False)


@pytest.mark.parametrize("scheme", ["single", "double"])
def test_keyset_item_pass_scalars_partial_sums_and_fail_word(scheme):
    keys, _ = vic.keyset(scheme)
    cases, runs = vic.keyset_cases(scheme), {}
    for case in cases:
        blocks = case["blocks"] or vic.own_grid(len(case["idx"]))
        want = vic.keyset_expected(scheme, case, blocks)
        grids = tuple(vic.grids_of(cases, case))
        key = (len(case["idx"]), case["c"], grids)
        if key not in runs:
            runs[key] = kvh.items(scheme, keys, case["idx"], case["b"], frc.PINNED_SEED, case["c"], grids)
        vic.compare((scheme, case["name"]), want, runs[key], blocks)
    assert len(runs) == len(vic.KEYSET_NS)
    vic.classes_populated(keysets=True)

"""The scalar arithmetic modulo the group order r on the device, with crafted inputs: tools/frcheck (the stage bodies of
tools/fr_stages.h, the same ones the CPU build runs in test_fr_host.py, one lane per item) run once in a subprocess under a
time limit, every output word checked with the Python code of tests/fr_cases.py against Python integers and a ChaCha20
written from RFC 8439 -- never against the CPU build.  Then, through the profiling build in a child process, the per-item passes
of the two verdict algorithms under the pinned seed: every scalar, block sum, total and the fail word (tests/verdict_item_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fr_cases as frc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "frcheck")


@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_tools()                                       # builds tools/frcheck when it is missing or stale
    assert os.path.exists(EXE)
    r = frc.build_records()
    d = tmp_path_factory.mktemp("frcheck")
    frc.input_words(r).tofile(d / "in.bin")
    p = subprocess.run([EXE, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = np.fromfile(d / "out.bin", np.uint32)
    assert len(out) == frc.output_words(r)
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


def test_item_passes_of_both_verdict_algorithms_under_the_pinned_seed():
    """fr_items_child.py loads the profiling build once: jjs_debug_verdict_items_dev and jjs_debug_keyset_items_dev over the cases
    of tests/verdict_item_cases.py (test_fr_host.py holds the same cases against the CPU build)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fr_items_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]
    print(p.stdout)

"""The affine key tables on the CPU build: tests/hostbuild/affine_tables_harness.cpp, a stand-alone program (with the host
sanitizers when JJS_HOST_SANITIZE=1 is set), runs the key-table stages of tools/scalar_stages.h on the records of
tests/affine_tables_cases.py -- both window widths, the points of the `kt tables` cases, the crafted scalars, the challenges at
their extremes -- and every output is compared with the Python oracle."""
import os
import subprocess

import numpy as np
import pytest

import affine_tables_cases as atc
import scalar_mul_cases as smc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostbuild", "affine_tables_harness.cpp")
SANITIZE = bool(os.environ.get("JJS_HOST_SANITIZE"))
EXE = os.path.join(HERE, "hostbuild", "affine_tables_harness" + ("_san" if SANITIZE else ""))     # one binary per kind of build
CSRC = os.path.join(ROOT, "jubjub_schnorr_amd", "csrc")


def build_harness():
    deps = [SRC, os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "scalar_stages.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if SANITIZE else ["-O2"]
        subprocess.check_call(["g++", *san, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", EXE, SRC])
    return EXE


@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    r = atc.build_records()
    d = tmp_path_factory.mktemp("affine_tables")
    smc.input_words(r).tofile(d / "in.bin")
    p = subprocess.run([build_harness(), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = np.fromfile(d / "out.bin", np.uint32)
    assert len(out) == atc.output_words(r)
    return atc.attach_outputs(r, out)


def test_every_entry_is_affine_and_the_multiple_of_its_base(recs):
    atc.check_tables_are_affine(recs)


def test_kt_add_scalar_on_the_crafted_scalars(recs):
    atc.check_scalars(recs)


def test_challenges_without_the_dead_position(recs):
    atc.check_challenges(recs)

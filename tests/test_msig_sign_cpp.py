"""jjs::multisig::sign_round_1 / sign_round_2 and CombineResult::first_failing_slot of the C++ header (include/jjs_schnorr.hpp) on the
reference's multisignature KAT (3 participants, extended points with Z != 1): without a GPU, sign_round_1's host arithmetic against
the fixture's points and the refusals of the host-side row search; on the GPU every signer's share against the KAT bytes, the two new
errors, and the failing slot of `combine`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_msig_sign.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_msig_sign")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def vector(tmp_path):
    import msig_sign_cases as sc
    with open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")) as f:
        kat = json.load(f)["multisig_kat"]
    c = sc.kat_case(kat)
    x = c.to_ext(41)
    z = np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in kat["individual_shares"]])
    fields = {"sk": c.sk, "r": c.r, "s": c.s, "pk": x.PK, "R": x.R, "S": x.S, "Ra": c.R, "Sa": c.S, "m": c.m[0], "z": z}
    path = tmp_path / "vector.txt"
    path.write_text("".join(f"{name} {np.ascontiguousarray(value).tobytes().hex()}\n" for name, value in fields.items()))
    return str(path)


def test_cpp_msig_sign_host_side(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    out = subprocess.run([build(tmp_path), vector(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "3 participants, host only, 0 failures" in out.stdout


@pytest.mark.gpu
def test_cpp_msig_sign_with_the_engine(tmp_path):
    out = subprocess.run([build(tmp_path), vector(tmp_path), "gpu"], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "3 participants, with the engine, 0 failures" in out.stdout

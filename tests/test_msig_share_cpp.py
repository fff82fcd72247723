"""jjs::multisig::verify_share, verify_share_batch, SignerGroup::verify_share and KeySet::multisig_verify_share of the C++ header
(include/jjs_schnorr.hpp) on the reference's multisignature KAT (3 participants, extended points with Z != 1 and their to_bytes
forms): without a GPU the answers the header makes on the host (index == len, unequal vectors, an empty transcript: no device call --
the engine is never initialised there); on the GPU every share verifies, a wrong share is InvalidMultisigShare carrying its index,
and sig_R is the KAT's aggregate commitment."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_msig_share.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_msig_share")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def vector(tmp_path):
    import jjs_oracle as o
    import msig_sign_cases as sc
    import msig_wire_cases as wc
    from helpers import to_pt
    with open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")) as f:
        kat = json.load(f)["multisig_kat"]
    c = sc.kat_case(kat)
    x = c.to_ext(43)
    z = np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in kat["individual_shares"]])
    rsa = o.decompress(bytes.fromhex(kat["aggregate_commitment"]))
    assert rsa is not None
    w = [wc.compress_column(a) for a in (c.PK, c.R, c.S)]
    assert [o.compress(to_pt(p)).hex() for p in c.PK] == kat["public_keys"]
    fields = {"pk": x.PK, "R": x.R, "S": x.S, "pkw": w[0], "Rw": w[1], "Sw": w[2], "pka": c.PK, "m": c.m[0], "z": z,
              "rsa": np.frombuffer(o.le32(rsa[0]) + o.le32(rsa[1]), np.uint8)}
    path = tmp_path / "vector.txt"
    path.write_text("".join(f"{name} {np.ascontiguousarray(value).tobytes().hex()}\n" for name, value in fields.items()))
    return str(path)


def test_cpp_msig_share_host_side(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    out = subprocess.run([build(tmp_path), vector(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "3 participants, host only, 0 failures" in out.stdout


@pytest.mark.gpu
def test_cpp_msig_share_with_the_engine(tmp_path):
    out = subprocess.run([build(tmp_path), vector(tmp_path), "gpu"], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "3 participants, with the engine, 0 failures" in out.stdout

"""jjs::multisig::combine and the extended SignerGroup of the C++ header (include/jjs_schnorr.hpp): compiles and links on CPU; on
the GPU it combines the transcript of the reference's multisignature known-answer test (tests/golden/reference_kat.json,
reference src/multisig.rs:544-672) in extended form -- u and RSa are the KAT's -- names the participant of a spoilt share, and
answers the two transcript errors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_msig_ext.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_msig_ext")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_multisig_combine_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.gpu
def test_cpp_multisig_combine_on_the_reference_kat_in_extended_form(tmp_path):
    import jjs_oracle as o
    import msig_ext_cases as xc
    from helpers import pt_bytes
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))["multisig_kat"]
    rng = np.random.default_rng(7)
    ext = lambda scalars: xc.to_ext_column(np.stack([pt_bytes(o.mul(o.G, s)) for s in scalars]), rng, xc.CHOSEN_Z).tobytes()  # noqa: E731
    sig = bytes.fromhex(k["signature"])
    agg, rsa = o.decompress(bytes.fromhex(k["aggregate_public_key"])), o.decompress(sig[32:])
    fields = {"pk": ext(k["secret_keys"]), "z": b"".join(bytes.fromhex(z) for z in k["individual_shares"]), "R": ext(k["r_scalars"]),
              "S": ext(k["s_scalars"]), "m": o.le32(k["message"]), "agg": pt_bytes(agg).tobytes(), "u": sig[:32], "rsa": pt_bytes(rsa).tobytes(),
              "spoil": bytes([1])}
    path = tmp_path / "transcript.txt"
    path.write_text("".join(f"{name} {value.hex()}\n" for name, value in fields.items()))
    out = subprocess.run([build(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "3 participants, 0 failures" in out.stdout

"""The overloads of jjs::multisig and SignerGroup in the C++ header (include/jjs_schnorr.hpp) that take `to_bytes` forms: compile
and link on CPU, beside the existing clients whose braced calls must keep meaning the extended forms; on the GPU they combine and
verify the reference's multisignature known answer (tests/golden/reference_kat.json, reference src/multisig.rs:544-672) from its
own wire bytes, name the participant of a spoilt share, and answer undecodable encodings."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path, name="test_msig_wire"):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_wire_overloads_compile_and_link(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.parametrize("client", ["test_msig_ext", "test_msig_verify"])
def test_the_braced_calls_of_the_existing_clients_still_compile(tmp_path, client):
    """combine({}, {}, {}, {}, m), aggregate_pk({}), verify({}, sig, m) and the braced verify_batch: the wire overloads do not
    make them ambiguous."""
    build(tmp_path, client)


@pytest.mark.gpu
def test_cpp_multisig_from_the_wire_bytes_of_the_reference_kat(tmp_path):
    import jjs_oracle as o
    import msig_wire_cases as wc
    from helpers import pt_bytes
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))["multisig_kat"]
    sig = bytes.fromhex(k["signature"])
    agg, rsa = o.decompress(bytes.fromhex(k["aggregate_public_key"])), o.decompress(sig[32:])
    cat = lambda xs: b"".join(bytes.fromhex(x) for x in xs)  # noqa: E731
    fields = {"pk": cat(k["public_keys"]), "z": cat(k["individual_shares"]), "R": cat(k["r_points"]), "S": cat(k["s_points"]),
              "m": o.le32(k["message"]), "sig": sig, "agg": pt_bytes(agg).tobytes(), "rsa": pt_bytes(rsa).tobytes(),
              "bad": wc.encoding("non-residue"), "spoil": bytes([1])}
    path = tmp_path / "transcript.txt"
    path.write_text("".join(f"{name} {value.hex()}\n" for name, value in fields.items()))
    out = subprocess.run([build(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "3 participants, 0 failures" in out.stdout

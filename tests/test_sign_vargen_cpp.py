"""jjs::SecretKeyVarGen of the C++ header (include/jjs_schnorr.hpp) on the reference's own bytes (tests/golden/reference_kat.json,
serde_secret_key_var_gen / serde_public_key_var_gen / serde_signature_var_gen): without a GPU the byte forms; on the GPU
public_key, sign and sign_batch for the affine and the wire key, and malformed keys."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_sign_vargen.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_sign_vargen")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def vector(tmp_path):
    import jjs_oracle as o
    import sign_vargen_pt_cases as vc
    from helpers import pt_bytes
    with open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")) as f:
        k = vc.kat(json.load(f))
    gen = o.decompress(k["secret"][32:])
    fields = {"secret": k["secret"], "public": k["public"], "signature": k["signature"], "m": k["m"].tobytes(), "rnd": k["rnd"].tobytes(),
              "gen": pt_bytes(gen).tobytes()}
    path = tmp_path / "vector.txt"
    path.write_text("".join(f"{name} {bytes(value).hex()}\n" for name, value in fields.items()))
    return str(path)


def test_cpp_sign_vargen_host_side(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    out = subprocess.run([build(tmp_path), vector(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "SecretKeyVarGen, host only, 0 failures" in out.stdout


@pytest.mark.gpu
def test_cpp_sign_vargen_with_the_engine(tmp_path):
    out = subprocess.run([build(tmp_path), vector(tmp_path), "gpu"], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "SecretKeyVarGen, with the engine, 0 failures" in out.stdout

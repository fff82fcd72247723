"""jjs::SecretKey of the C++ header (include/jjs_schnorr.hpp) on the reference's own bytes (tests/golden/reference_kat.json,
serde_secret_key / serde_public_key / serde_public_key_double / serde_signature / serde_signature_double): without a GPU the
byte forms and the range test of from_bytes; on the GPU public_key, public_key_double, sign, sign_double and the batches, and
refused items."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_sign_fixed.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_sign_fixed")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def vector(tmp_path):
    import sign_fixed_cases as fc
    with open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")) as f:
        k = fc.kat(json.load(f))
    fields = {name: k[name] for name in ("secret", "public", "public_double", "signature", "signature_double")}
    fields.update({name: k[name].tobytes() for name in ("m", "rnd", "rnd_double")})
    path = tmp_path / "vector.txt"
    path.write_text("".join(f"{name} {bytes(value).hex()}\n" for name, value in fields.items()))
    return str(path)


def test_cpp_sign_fixed_host_side(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    out = subprocess.run([build(tmp_path), vector(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "SecretKey, host only, 0 failures" in out.stdout


@pytest.mark.gpu
def test_cpp_sign_fixed_with_the_engine(tmp_path):
    out = subprocess.run([build(tmp_path), vector(tmp_path), "gpu"], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "SecretKey, with the engine, 0 failures" in out.stdout

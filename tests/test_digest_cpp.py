"""jjs::poseidon::digest, digest_truncated and digest_batch of the C++ header (include/jjs_schnorr.hpp).  On the CPU the test
program is built against a recording stand-in of jjs_digest and checks what the header marshals (the column, the offsets, the
flag, status -> optional), and it links against the engine; on the GPU it digests known payloads."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_digest.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC]


def build(tmp_path):
    exe = str(tmp_path / "test_digest")
    subprocess.check_call(CXX + ["-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_marshalling(tmp_path):
    exe = str(tmp_path / "test_digest_stub")
    subprocess.check_call(CXX + ["-DJJS_STUB", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "0 failures" in out.stdout


def test_cpp_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.gpu
def test_cpp_known_payloads(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "0 failures" in out.stdout

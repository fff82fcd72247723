"""`is_valid` of the C++ header (include/jjs_schnorr.hpp): is_valid() on the six types and jjs::is_valid_batch.  On the CPU the
test program is built against a recording stand-in of the two host calls and checks what the header marshals (columns, widths,
scheme, format, the outputs it asks for, status -> bool), and it links against the engine; on the GPU it checks known points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_points_check.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC]


def build(tmp_path):
    exe = str(tmp_path / "test_points_check")
    subprocess.check_call(CXX + ["-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_marshalling(tmp_path):
    exe = str(tmp_path / "test_points_check_stub")
    subprocess.check_call(CXX + ["-DJJS_STUB", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "0 failures" in out.stdout


def test_cpp_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.gpu
def test_cpp_known_points(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "0 failures" in out.stdout

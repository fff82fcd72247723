"""jjs::KeySet::remove / compact / removal of the C++ header (include/jjs_schnorr.hpp): compiles and links on CPU; on the GPU
tests/cpp/test_keyset_remove.cpp registers the keys of the single-scheme golden vectors, removes every second one, compacts and
verifies."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_keyset_remove.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_keyset_remove")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L" + PKG, "-l:libjjs_gpu.so", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_keyset_remove_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.gpu
def test_cpp_keyset_remove_golden_vectors(tmp_path):
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "verify_vectors.json")))["single"]
    lines = [" ".join([v["name"], str(v["status"])] + [v[k] for k in ("u", "R", "PK", "m")]) for v in vec]
    assert len(lines) >= 4
    path = tmp_path / "vectors.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([build(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert f"{len(lines)} vectors, 0 failures" in out.stdout

"""jjs::KeySet::multisig_combine of the C++ header (include/jjs_schnorr.hpp): compiles and links on CPU; on the GPU it registers
the 16 keys of msig_keyset_cases.key_set and combines one transcript of four of them from extended points: the signature is the
oracle's, a spoilt share is InvalidMultisigShare(1), a row naming an unusable key or an index outside the set is BytesError(2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_msig_keyset.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_msig_keyset")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_keyset_multisig_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.gpu
def test_cpp_keyset_multisig_good_spoilt_and_refused(tmp_path):
    import msig_keyset_cases as kcs
    import multisig_cases as mc
    keys, sk = kcs.key_set()
    kc = kcs.pool_transcripts([4], 950, keys, sk)
    e = mc.expected(kc.case)
    assert e.ts.tolist() == [0]
    d = kc.case.dirty
    fields = {"keys": keys, "status": np.array(kcs.KEY_STATUS, np.uint8), "idx": kc.key_idx.astype("<u4"), "z": d["z"], "R": kcs.to_ext(d["R"]),
              "S": kcs.to_ext(d["S"]), "m": d["m"], "u": e.su[0], "rsa": e.sr[0], "bad": np.array([kcs.ORDER8_KEY], "<u4")}
    path = tmp_path / "transcript.txt"
    path.write_text("".join(f"{name} {np.ascontiguousarray(value).tobytes().hex()}\n" for name, value in fields.items()))
    out = subprocess.run([build(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "16 keys, 4 participants, 0 failures" in out.stdout

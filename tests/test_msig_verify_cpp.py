"""jjs::multisig::aggregate_pk / verify / verify_batch and jjs::KeySet::multisig_aggregate_pk / multisig_verify of the C++ header
(include/jjs_schnorr.hpp): compiles and links on CPU; on the GPU one vector of four of msig_keyset_cases.key_set's keys from
extended points: the aggregate is the oracle's and the signature verifies, a spoilt u is InvalidSignature, a vector with an
unusable key is refused (BytesError, no aggregate), the empty vector aggregates to the identity."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_msig_verify.cpp")
PKG = os.path.join(ROOT, "jubjub_schnorr_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_msig_verify")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           SRC, "-o", exe, "-L" + PKG, "-l:libjjs_gpu.so", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_msig_verify_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libjjs_gpu.so")), "run __graft_entry__.build() first"
    build(tmp_path)


@pytest.mark.gpu
def test_cpp_msig_verify_good_spoilt_and_refused(tmp_path):
    import msig_ext_cases as xc
    import msig_keyset_cases as kcs
    import msig_verify_cases as vc
    keys, sk = kcs.key_set()
    c = vc.build([[7, 1, 10, 4]], 1500, keys, sk)
    agg, vst, st, tally = vc.expected(c)
    assert st.tolist() == [0] and vst.tolist() == [0]
    pk_ext = xc.to_ext_column(c.PK, np.random.default_rng(1501), xc.CHOSEN_Z)
    fields = {"keys": keys, "idx": c.key_idx.astype("<u4"), "pk": pk_ext, "u": c.u[0], "R": c.R[0], "m": c.m[0], "agg": agg[0],
              "bad": np.array([kcs.ORDER8_KEY], "<u4")}
    path = tmp_path / "vector.txt"
    path.write_text("".join(f"{name} {np.ascontiguousarray(value).tobytes().hex()}\n" for name, value in fields.items()))
    out = subprocess.run([build(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "16 keys, 4 in the vector, 0 failures" in out.stdout

"""The scalar multiplications on the device with crafted scalars and points: tools/scalarcheck (the stage bodies of
tools/scalar_stages.h, the same ones the CPU build runs in test_scalar_mul_host.py, plus the quad chains that only the device
has) run once in a subprocess under a time limit, every output checked with the Python code of tests/scalar_mul_cases.py
against the oracle's big-integer curve arithmetic.  Then, through the ABI with the library's own tables: public-key derivation
on the whole comb list, the per-item-generator signer's key on the whole list of the 4-bit windows, and valid signatures whose
points coincide (PK = +-G, PK = +-R, Gen = G, PK = Gen) on the latency path; tests/forcepath_child.py runs the same items on
the throughput path and through the key tables of both widths."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import jjs_oracle as o
import scalar_mul_cases as smc
from helpers import ARG_ORDER, fe_arr, oracle_verify, pt_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "scalarcheck")


@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_tools()                                       # builds tools/scalarcheck when it is missing or stale
    assert os.path.exists(EXE)
    r = smc.build_records(device=True)
    d = tmp_path_factory.mktemp("scalarcheck")
    smc.input_words(r).tofile(d / "in.bin")
    p = subprocess.run([EXE, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = np.fromfile(d / "out.bin", np.uint32)
    assert len(out) == smc.output_words(r)
    return smc.attach_outputs(r, out)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_case_classes_are_all_populated(recs):
    assert smc.CLASS_COUNTS and all(v > 0 for k, v in smc.CLASS_COUNTS.items() if not k.endswith("clamped")), smc.CLASS_COUNTS
    assert len(recs) == 18


def test_comb_mul(recs):
    smc.check_comb(recs)


def test_table_mul(recs):
    smc.check_table(recs)


def test_check_equation_fixed_and_per_item_generator(recs):
    smc.check_equations(recs)


def test_key_tables_both_widths_and_quad_chains(recs):
    assert "kt bases quad w=5" in recs and "kt bases quad w=6" in recs
    smc.check_kt(recs)


def test_latency_path_pieces_tables_and_quad_chains(recs):
    assert all("sb tables quad positions=%d" % p in recs for p in (4, 8, 16))
    smc.check_latency_path(recs)


def test_public_keys_on_the_comb_scalars(eng):
    """derive_kernel -> comb_mul on the library's own tables: every scalar of the 16-bit list, both generators"""
    sks = [s for _, s in smc.scalars(16, random.Random(16))]
    PK, PKp, bad = (t.cpu().numpy() for t in eng.public_keys(dev(fe_arr(sks)), double=True))
    assert not bad.any()
    for i, s in enumerate(sks):
        assert PK[i].tobytes() == pt_bytes(o.mul(o.G, s)).tobytes(), hex(s)
        assert PKp[i].tobytes() == pt_bytes(o.mul(o.G_NUMS, s)).tobytes(), hex(s)


def test_vargen_signer_key_on_the_window_scalars(eng):
    """sign_kernel -> build_point_table + table_mul: PK = sk * (g * G) for every scalar of the 4-bit list"""
    prng = random.Random(4)
    sks = [s for _, s in smc.scalars(4, prng)]
    gs = [(1, 2, smc.R - 1, prng.randrange(1, smc.R))[i % 4] for i in range(len(sks))]
    n = len(sks)
    rnd, m = fe_arr([prng.randrange(smc.R) for _ in range(n)]), fe_arr([prng.randrange(smc.Q) for _ in range(n)])
    u, R_, PK, Gen = (t.cpu().numpy() for t in eng.sign("vargen", dev(fe_arr(sks)), dev(rnd), dev(m), gen_scalar=dev(fe_arr(gs))))
    gens = {g: o.mul(o.G, g) for g in set(gs)}
    for i, (s, g) in enumerate(zip(sks, gs)):
        assert Gen[i].tobytes() == pt_bytes(gens[g]).tobytes(), (hex(s), g)
        assert PK[i].tobytes() == pt_bytes(o.mul(gens[g], s)).tobytes(), (hex(s), g)


@pytest.mark.parametrize("scheme", ["single", "double", "vargen"])
def test_coinciding_points_on_the_latency_path(eng, scheme):
    b = smc.degenerate_batch(scheme)
    want, want_c = oracle_verify(scheme, b, want_c=True)
    assert set(want.tolist()) == {0, 2}
    args = [dev(b[k]) for k in ARG_ORDER[scheme]]
    before = eng.path_stats()
    st, tally = eng.verify(scheme, *args)
    c = eng.challenge(scheme, *args[1:])
    assert st.cpu().numpy().tolist() == want.tolist()
    assert tally.cpu().numpy().tolist() == [int((want == k).sum()) for k in range(4)]
    assert (c.cpu().numpy() == want_c).all()
    after = eng.path_stats()
    assert after["latency"] > before["latency"] and after["throughput"] == before["throughput"], (before, after)   # by its size

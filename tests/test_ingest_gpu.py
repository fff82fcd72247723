"""Inversion, inverse square roots, point decoding and the normalisation of extended coordinates on the device with the crafted
inputs of tests/ingest_cases.py: tools/ingestcheck (the stage bodies of tools/ingest_stages.h, the same ones the CPU build runs
in test_ingest_host.py) run once in a subprocess under a time limit, every output word checked with Python integers.  Then the
engine's own square-root tables, all 7 x 256 powers and 65 536 bytes, against Python, against the CPU build of the same source
bit for bit, and against the tool's; and through the ABI: jjs_decompress_dev at the sizes where decode_kernel changes its
course (one item, around a wave, around a block, past its grid limit so that the grid-stride loop runs, none), and the crafted
encodings as R and as PK of jjs_verify_single_wire on the latency path (512 items, decode_points_kernel) and above it
(17 008 items).

Division steps (ingest_cases.RECORDED, held against every run): over the 2 816 inversion inputs, crafted and random, with the
longest that a seeded search finds, an input needs between 501 and 531 steps, 514 on average; fq_inverse does 600, and nothing
here can tell 20 batches from 19."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hostlib as hl
import ingest_cases as ic
import jjs_oracle as o
from helpers import fe_arr, pt_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "ingestcheck")
BLOCK = 256                                  # csrc/device_kernels.h
GRID_LIMIT = 8192                            # launch_decode


@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_tools()                                       # builds tools/ingestcheck when it is missing or stale
    assert os.path.exists(EXE)
    r = ic.build_records()
    d = tmp_path_factory.mktemp("ingestcheck")
    ic.input_words(r).tofile(d / "in.bin")
    p = subprocess.run([EXE, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = np.fromfile(d / "out.bin", np.uint32)
    assert len(out) == ic.output_words(r)
    return ic.attach_outputs(r, out)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


@pytest.fixture(scope="module")
def crafted():
    """the crafted encodings (n, 32), the oracle's affine bytes (n, 64) and ok (n,)"""
    cases, want = ic.decompress_cases()
    aff, ok = ic.decompress_expected_bytes(want)
    return np.frombuffer(b"".join(e for _, e in cases), np.uint8).reshape(-1, 32).copy(), aff, ok


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_case_classes_are_all_populated(recs):
    assert ic.CLASS_COUNTS and all(v > 0 for k, v in ic.CLASS_COUNTS.items() if k != ic.NEGATIVE_D), ic.CLASS_COUNTS
    assert len(recs) == 34
    assert ic.DRAWS["drawn"] < 8192


def test_recorded_figures_are_those_of_this_run(recs):
    """the step counts and case counts that DESIGN.md 6.8 and the docstring above quote (ingest_cases.RECORDED) are what this
    run finds; no bound on the step count is set"""
    print("division steps over the inversion inputs:", ic.STEP_STATS)
    ic.check_recorded()


def test_one_batch_applied_to_d_and_e(recs):
    ic.check_update(ic.update_cases(), recs["one batch applied to d and e"]["out"].reshape(-1, 20))


def test_inverse(recs):
    ic.check_inv(ic.inversion_cases(), recs["inverse"]["out"].reshape(-1, 8))


def test_end_of_the_inversion(recs):
    ic.check_finish(ic.finish_cases(), recs["end of the inversion"]["out"].reshape(-1, 10))


def test_inverse_square_root(recs):
    ic.check_inv_sqrt(ic.inv_sqrt_cases(), recs["inverse square root"]["out"].reshape(-1, 8))


def test_decompress(recs):
    cases, want = ic.decompress_cases()
    out = recs["decompress"]["out"].reshape(-1, 20)
    assert not out[:, 17:].any()
    ic.check_decompress(cases, want, np.ascontiguousarray(out[:, :16]).view(np.uint8).reshape(-1, 64), out[:, 16])


def test_normalize(recs):
    n = 0
    for r in recs.values():
        if r["kind"] == "K_NORMALIZE":
            ic.check_normalize(r)
            n += 1
    assert n == len(ic.normalize_records()) == 28


def host_tables():
    r = [x for x in ic.build_records() if x["kind"] == "K_TABLES"]
    return ic.table_dump(ic.attach_outputs(r, hl.ingest_records(ic.input_words(r), ic.output_words(r)))["tables"])


def test_dlog_tables(eng):
    """the engine's own tables (dlog_table_kernel after a hipMemsetAsync): every entry against Python, every limb against the
    CPU build of the same source"""
    pw, hs = eng.debug_dlog_tables()
    ic.check_tables(pw, hs, same_as=host_tables())


def test_tool_tables_are_the_engines(recs, eng):
    pw, hs = ic.table_dump(recs["tables"])
    ic.check_tables(pw, hs, same_as=eng.debug_dlog_tables())


def tiled(a, n):
    return a[np.arange(n) % len(a)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, None])
def test_decompress_dev_sizes(eng, crafted, n):
    """n items of the crafted set (None: all of them) through decode_kernel, compared with the oracle; the accepted ones go back
    through compress_kernel to their input bytes"""
    enc, aff, ok = crafted
    n = len(enc) if n is None else n
    rot = (7 * n) % len(enc)                       # another stretch of the set for every size
    e, a, k = (tiled(np.roll(x, -rot, 0), n) for x in (enc, aff, ok))
    got_aff, got_ok = eng.decompress(dev(e))
    back = eng.compress(got_aff).cpu().numpy()
    got_aff, got_ok = got_aff.cpu().numpy(), got_ok.cpu().numpy()
    assert np.array_equal(got_ok, k), np.nonzero(got_ok != k)[0][:8]
    assert np.array_equal(got_aff, a), np.nonzero((got_aff != a).any(1))[0][:8]
    acc = k == 1
    assert np.array_equal(back[acc], e[acc])
    if n == len(enc):
        cases, want = ic.decompress_cases()
        ic.check_decompress(cases, want, np.roll(got_aff, rot, 0), np.roll(got_ok, rot, 0))


def test_decompress_dev_grid_stride(eng, crafted):
    """more items than the 8192 blocks of decode_kernel's grid hold: the lanes go round their loop a second time"""
    enc, aff, ok = crafted
    n = GRID_LIMIT * BLOCK + 65
    got_aff, got_ok = eng.decompress(dev(tiled(enc, n)))
    got_aff, got_ok = got_aff.cpu().numpy(), got_ok.cpu().numpy()
    assert np.array_equal(got_ok, tiled(ok, n))
    assert np.array_equal(got_aff, tiled(aff, n))


def test_decompress_dev_of_nothing(eng, crafted):
    import torch
    enc = dev(crafted[0][:4])
    out, ok = torch.full((4, 64), 0x5A, dtype=torch.uint8).cuda(), torch.full((4,), 0x5A, dtype=torch.uint8).cuda()
    rc = eng._lib.jjs_decompress_dev(ctypes.c_void_p(enc.data_ptr()), 0, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ok.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all() and (ok.cpu().numpy() == 0x5A).all()


def wire_items(enc, aff, ok, sel):
    """every chosen encoding once as R and once as PK beside the generator: wire arrays, affine arrays, decodable flags"""
    prng = np.random.default_rng(0x31CE)
    g_enc, g_aff = np.frombuffer(o.compress(o.G), np.uint8), pt_bytes(o.G)
    m = len(sel)
    R = np.concatenate([enc[sel], np.tile(g_enc, (m, 1))]); PK = np.concatenate([np.tile(g_enc, (m, 1)), enc[sel]])
    Ra = np.concatenate([aff[sel], np.tile(g_aff, (m, 1))]); PKa = np.concatenate([np.tile(g_aff, (m, 1)), aff[sel]])
    u = fe_arr([int.from_bytes(prng.bytes(40), "little") % o.R_ORDER for _ in range(2 * m)])
    msg = fe_arr([int.from_bytes(prng.bytes(40), "little") % o.Q for _ in range(2 * m)])
    return u, R, PK, msg, Ra, PKa, np.concatenate([ok[sel], ok[sel]])


@pytest.mark.parametrize("size", ["latency path", "above it"])     # decode_points_kernel, then decode_kernel and the key decoding
def test_crafted_encodings_through_verify_single_wire(eng, crafted, size):
    """status 3 exactly where the oracle cannot decode; elsewhere the status of the affine call on the decoded points"""
    enc, aff, ok = crafted
    cases, _ = ic.decompress_cases()
    if size == "latency path":                        # 256 encodings, 512 items: every small class whole, the two long ones thinned
        long_cls = ("random valid, every byte of k", "small v without a root, every odd k0")
        sel = [i for i, (c, _) in enumerate(cases) if c not in long_cls]
        take = (256 - len(sel)) // 2
        for c in long_cls:
            idx = [i for i, (c2, _) in enumerate(cases) if c2 == c]
            sel += idx[::len(idx) // take][:take]
        sel = np.array(sorted(sel))
        assert len(sel) <= 256 and (ok[sel] == 0).sum() >= 32 and (ok[sel] == 1).sum() >= 64
    else:                                             # the whole set four times: more than the 16 384 items the latency path takes
        sel = np.tile(np.arange(len(enc)), 4)
        assert 2 * len(sel) > 16384
    u, R, PK, msg, Ra, PKa, decodable = wire_items(enc, aff, ok, sel)
    assert (len(u) <= 512) == (size == "latency path")
    before = eng.path_stats()
    st, tally = eng.verify_wire("single", dev(np.concatenate([u, R], 1)), dev(PK), dev(msg))
    st = st.cpu().numpy()
    after = eng.path_stats()
    assert (after["latency"] > before["latency"]) == (size == "latency path"), (before, after)
    want, _ = eng.verify("single", dev(u), dev(Ra), dev(PKa), dev(msg))
    want = want.cpu().numpy().copy()
    assert not (want[decodable == 1] == 3).any()
    want[decodable == 0] = 3
    assert np.array_equal(st, want), np.nonzero(st != want)[0][:8]
    assert tally.cpu().numpy().tolist() == [int((want == k).sum()) for k in range(4)]

"""The extended-coordinate and host-buffer forms of the multisignature calls on the device (jjs_multisig_combine_ext_dev,
jjs_msig_group_create_ext, jjs_msig_group_combine_ext_dev, jjs_multisig_combine, jjs_msig_group_combine).  Every extended
device call is compared two ways: byte for byte, every output, with the affine device call on the derived columns of
msig_ext_cases.py in the same process; and with jjs_oracle_c.multisig_combine through multisig_cases.check under its 2 % cap.
A call too small to hold a planted point under that cap is compared with the affine call alone, and with the oracle on clean
inputs.  Timing is asserted nowhere."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import jjs_oracle as o
import msig_ext_cases as xc
import msig_ext_child as child
import msig_group_cases as gcs
import multisig_cases as mc
from helpers import ARG_ORDER, make_batch, oracle_verify

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = 16
LANES_ONE_ROW = 131072           # launch_normalize: one row per lane up to here, several beyond


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(outs):
    import torch
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in outs)


def same(a, b, label, names=mc.OUTPUTS):
    assert len(a) == len(b) == len(names)
    for k, x, y in zip(names, a, b):
        assert x.shape == y.shape and (x == y).all(), (label, k, np.nonzero((x != y).reshape(len(x), -1).any(1))[0][:8].tolist())


def ext_call(eng, x):
    a = x.args()
    return host(eng.multisig_combine(*[dev(c) for c in a[:5]], a[5], fmt="ext"))


def affine_call(eng, case):
    a = case.args()
    return host(eng.multisig_combine(*[dev(c) for c in a[:5]], a[5]))


def two_ways(eng, x, label, oracle=True):
    got = ext_call(eng, x)
    same(got, affine_call(eng, x.derived), label + ": extended call against the affine call on the derived columns")
    uncompared = mc.check(x.derived, mc.expected(x.derived, THREADS), got, label) if oracle else None
    print(f"ext call {label}: shares={x.n} T={x.T} planted={len(x.plants)} uncompared={uncompared}")
    for t, j, _, _ in x.plants:
        assert got[0][x.derived.row(t, j)] == 3 and got[4][t] != 0 and not got[2][t].any() and not got[3][t].any(), (label, t, j)
    return got


# ---- the inline call ----
def test_eight_shares_in_one_transcript(eng):
    """One row per lane, eight hash lanes.  Too small for a planted point under the cap: with plants against the affine call,
    clean against the oracle."""
    clean = xc.ExtCase(mc.valid_transcripts([8], seed=801, threads=THREADS), seed=802)
    got = two_ways(eng, clean, "8 shares, clean")
    assert got[0].tolist() == [0] * 8 and got[4].tolist() == [0]
    x = xc.ExtCase(mc.valid_transcripts([8], seed=801, threads=THREADS), seed=802)
    x.plant(0, 0, "PK", "Z=0"); x.plant(0, 3, "R", "U=q"); x.plant(0, 7, "S", "Z=2^256-1")
    two_ways(eng, x, "8 shares, planted", oracle=False)


def test_8193_shares_every_kind_in_every_column(eng):
    x = xc.ExtCase(mc.filler(8193, seed=811, threads=THREADS), seed=812)
    xc.plant_everywhere(x, boundary=x.T // 2)
    x.check_derived()
    two_ways(eng, x, "8193 shares")


def concat_expected(parts):
    """multisig_cases.Expected of mc.concat(cases) from [(Expected, case)] of its parts."""
    e, T = mc.Expected(), 0
    for k in ("st", "ts", "cmp_share", "cmp_agg", "ts_exact", "agg", "su", "sr"):
        setattr(e, k, np.concatenate([getattr(x, k) for x, _ in parts]))
    e.coord_transcripts = set()
    for x, case in parts:
        e.coord_transcripts |= {t + T for t in x.coord_transcripts}
        T += case.T
    e.uncompared = sum(x.uncompared for x, _ in parts)
    return e


def test_more_rows_than_lanes(eng):
    """131 072 + 300 shares: sixteen copies of a call of 8 192 (mc.tile) and a tail of 300, so that the lanes 0 .. 299 own two
    rows.  Planted points in rows below 300 and in rows >= 131 072, row 0 and row 131 072 among them: both rows of lane 0.  The
    oracle runs on the two parts, its results are tiled as the inputs are."""
    base = xc.ExtCase(mc.filler(8192, seed=821, threads=THREADS), seed=822)
    tail = xc.ExtCase(mc.filler(300, seed=823, threads=THREADS), seed=824)
    base.plant(0, 0, "PK", "Z=0"); base.plant(0, 0, "S", "V=q+1"); base.plant(40, 0, "R", "Z=0")
    assert base.derived.row(40, 0) < 300
    tail.plant(0, 0, "R", "Z=q"); tail.plant(0, 0, "S", "U=q")
    tail.plant(tail.T - 1, int(tail.derived.sizes()[-1]) - 1, "PK", "Z=2^256-1")
    reps = LANES_ONE_ROW // 8192
    x = xc.concat_ext(xc.tile_ext(base, reps), tail)
    assert x.n == LANES_ONE_ROW + 300 and x.derived.row(x.T - tail.T, 0) == LANES_ONE_ROW
    tiled = mc.tile(base.derived, reps)
    e = concat_expected([(mc.tile_expected(mc.expected(base.derived, THREADS), reps, base.T), tiled), (mc.expected(tail.derived, THREADS), tail.derived)])
    got = ext_call(eng, x)
    same(got, affine_call(eng, x.derived), "131072 + 300 shares: extended call against the affine call")
    uncompared = mc.check(x.derived, e, got, "131072 + 300 shares")
    print(f"ext call 131072 + 300 shares: T={x.T} planted={len(x.plants)} uncompared={uncompared}")
    for t, j, _, _ in x.plants:
        assert got[0][x.derived.row(t, j)] == 3 and got[4][t] != 0, (t, j)


def test_transcripts_of_256_and_257_participants(eng):
    sizes = [3, 256, 257, 2]
    clean = xc.ExtCase(mc.valid_transcripts(sizes, seed=831, threads=THREADS), seed=832)
    clean.derived.corrupt(2, 256)
    two_ways(eng, clean, "256 | 257, clean")
    x = xc.ExtCase(mc.valid_transcripts(sizes, seed=831, threads=THREADS), seed=832)
    x.plant(1, 255, "S", "Z=0"); x.plant(2, 0, "PK", "Z=q"); x.plant(2, 128, "R", "V=q+1")
    two_ways(eng, x, "256 | 257, planted", oracle=False)


def test_an_empty_transcript_first_and_last(eng):
    sizes = [0, 3, 0, 0, 5, 1, 0]
    clean = xc.ExtCase(mc.valid_transcripts(sizes, seed=841, threads=THREADS), seed=842)
    got = two_ways(eng, clean, "empty first and last, clean")
    assert got[4].tolist() == [5, 0, 5, 5, 0, 0, 5]
    x = xc.ExtCase(mc.valid_transcripts(sizes, seed=841, threads=THREADS), seed=842)
    x.plant(1, 0, "R", "Z=0"); x.plant(5, 0, "PK", "U=q")
    got = two_ways(eng, x, "empty first and last, planted", oracle=False)
    assert got[4].tolist() == [5, 3, 5, 5, 0, 3, 5]
    none = xc.ExtCase(mc.valid_transcripts([0, 0], seed=843, threads=THREADS), seed=844)
    assert two_ways(eng, none, "only empty transcripts")[4].tolist() == [5, 5]


# ---- signer groups ----
@functools.lru_cache(None)
def group_case(n):
    gc = gcs.group_transcripts(n, 64, seed=850 + n, threads=THREADS)
    pk_ext = xc.to_ext_column(gc.PK, np.random.default_rng(860 + n), xc.CHOSEN_Z[:min(n, 3)])
    return gc, pk_ext


@pytest.mark.parametrize("n", [1, 8, 257])
def test_group_calls(eng, n):
    """B = 1, 63, 64: both sides of the lane-mapping boundary.  The group from extended keys is the group from affine keys."""
    full, pk_ext = group_case(n)
    with eng.multisig_group(pk_ext, fmt="ext") as gx, eng.multisig_group(full.PK) as ga:
        assert (gx.aggregate_pk == ga.aggregate_pk).all()
        for B in (1, 63, 64):
            gc = full.slice(0, B)
            names = ("share_status", "sig_u", "sig_R", "transcript_status")
            clean = xc.ExtCase(gc.case, seed=870 + B)
            z, m = dev(gc.case.dirty["z"]), dev(gc.case.dirty["m"])
            got = host(gx.combine(z, dev(clean.ext["R"]), dev(clean.ext["S"]), m, fmt="ext"))
            want = host(ga.combine(z, dev(gc.case.dirty["R"]), dev(gc.case.dirty["S"]), m))
            same(got, want, f"group n={n} B={B} clean", names)
            same(got, host(ga.combine(z, dev(clean.ext["R"]), dev(clean.ext["S"]), m, fmt="ext")), f"affine group, ext call n={n} B={B}", names)
            mc.check(gc.case, mc.expected(gc.case, THREADS), gcs.as_inline_outputs(gc, gx.aggregate_pk, got), f"group n={n} B={B}")
            assert (got[3] == 0).all()
            x = xc.ExtCase(gc.case, seed=870 + B)
            x.plant(B - 1, n - 1, "R", "Z=0"); x.plant(0, 0, "S", "U=q")
            got = host(gx.combine(z, dev(x.ext["R"]), dev(x.ext["S"]), m, fmt="ext"))
            want = host(ga.combine(z, dev(x.derived.dirty["R"]), dev(x.derived.dirty["S"]), m))
            same(got, want, f"group n={n} B={B} planted", names)
            assert got[0][0] == 3 and got[0][-1] == 3 and got[3][0] == 3 and got[3][B - 1] != 0 and not got[1][0].any()


def test_a_registration_with_an_unusable_key_is_refused(eng):
    from jubjub_schnorr_amd import _ffi
    _, pk_ext = group_case(8)
    for j, kind in zip((0, 3, 7, 7, 1), xc.KINDS):
        spoilt = pk_ext.copy()
        xc.spoil(spoilt[j], kind)
        with pytest.raises(_ffi.JjsError, match="code -1"):
            eng.multisig_group(spoilt, fmt="ext")


# ---- state ----
def test_scratch_large_ext_then_small_ext_then_affine(eng):
    """The scratch grows for an extended call and is carved again; an affine call behind it gives the bytes a fresh process
    gives, whose scratch no extended call has touched."""
    big = xc.ExtCase(mc.filler(9001, seed=881, top=4, threads=THREADS), seed=882)
    xc.plant_everywhere(big, boundary=big.T // 2)
    two_ways(eng, big, "scratch: large ext")
    small = xc.ExtCase(mc.filler(301, seed=883, threads=THREADS), seed=884)
    two_ways(eng, small, "scratch: small ext")
    mine = child.digest(affine_call(eng, child.scratch_case()))
    out = subprocess.run([sys.executable, os.path.join(HERE, "msig_ext_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"digest {mine}" in out.stdout, "the affine call after extended calls against the affine call of a fresh process"


def test_prefilled_outputs_and_no_transcript_status(eng):
    import torch
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    x = xc.ExtCase(mc.filler(500, seed=891, threads=THREADS), seed=892)
    x.plant(3, 0, "R", "Z=0")
    want = ext_call(eng, x)
    a = x.args()
    ins = [dev(c) for c in a[:5]]
    full = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    st, ts, agg, su, sr = full(x.n), full(x.T), full(x.T, 64), full(x.T, 32), full(x.T, 64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.jjs_multisig_combine_ext_dev(*[p(t) for t in ins], a[5].ctypes.data_as(ctypes.c_void_p), x.T, p(st), None, p(agg), p(su), p(sr),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.jjs_last_error()
    got = host((st, agg, su, sr, ts))
    same(got[:4], want[:4], "prefilled outputs", mc.OUTPUTS[:4])
    assert (got[4] == 0xA5).all(), "transcript_status = NULL: nothing is written there"


def test_a_second_stream_beside_a_verify(eng):
    import torch
    x = xc.ExtCase(mc.filler(3001, seed=901, threads=THREADS), seed=902)
    xc.plant_everywhere(x, boundary=x.T // 2)
    want = ext_call(eng, x)
    b = make_batch("single", 20000, seed=903, n_keys=16)
    v_want = oracle_verify("single", b)
    v_args = [dev(b[k]) for k in ARG_ORDER["single"]]
    a = x.args()
    ins = [dev(c) for c in a[:5]]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    st, _ = eng.verify("single", *v_args)
    with torch.cuda.stream(side):
        outs = eng.multisig_combine(*ins, a[5], fmt="ext")
    st2, _ = eng.verify("single", *v_args)
    got = host(outs)
    same(got, want, "second stream")
    assert (st.cpu().numpy() == v_want).all() and (st2.cpu().numpy() == v_want).all()


# ---- the host forms ----
def test_host_forms_against_device_forms(eng):
    x = xc.ExtCase(mc.filler(2001, seed=911, threads=THREADS), seed=912)
    xc.plant_everywhere(x, boundary=x.T // 2)
    want = ext_call(eng, x)
    eng.trim()
    before = eng.memory_stats()["host_staging"]
    same(eng.multisig_combine(*x.args(), fmt="ext"), want, "host ext against device ext")
    same(eng.multisig_combine(*x.derived.args()), want, "host affine against device ext")
    grown = eng.memory_stats()["host_staging"]
    assert grown >= before + 3 * 96 * x.n, "the staging of the host form is reported"
    eng.trim()
    assert eng.memory_stats()["host_staging"] == before, "jjs_trim frees it"
    same(eng.multisig_combine(*x.args(), fmt="ext"), want, "host ext after a trim")
    # unaligned host pointers, and no transcript_status
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    a = x.args()
    odd = []
    for c in a[:5]:
        buf = np.zeros(c.size + 1, np.uint8)
        buf[1:] = c.reshape(-1)
        odd.append(buf[1:].reshape(c.shape))
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st, agg, su, sr = np.full(x.n, 0xA5, np.uint8), np.full((x.T, 64), 0xA5, np.uint8), np.full((x.T, 32), 0xA5, np.uint8), np.full((x.T, 64), 0xA5, np.uint8)
    assert lib.jjs_multisig_combine(1, *[p(c) for c in odd], p(a[5]), x.T, p(st), None, p(agg), p(su), p(sr)) == 0, lib.jjs_last_error()
    same((st, agg, su, sr), want[:4], "host ext, odd addresses", mc.OUTPUTS[:4])
    # the group
    full, pk_ext = group_case(8)
    gx = xc.ExtCase(full.case, seed=913)
    gx.plant(10, 2, "S", "Z=q")
    d = gx.derived.dirty
    with eng.multisig_group(pk_ext, fmt="ext") as g:
        names = ("share_status", "sig_u", "sig_R", "transcript_status")
        gwant = host(g.combine(dev(d["z"]), dev(gx.ext["R"]), dev(gx.ext["S"]), dev(d["m"]), fmt="ext"))
        same(g.combine(d["z"], gx.ext["R"], gx.ext["S"], d["m"], fmt="ext"), gwant, "group host ext", names)
        same(g.combine(d["z"], d["R"], d["S"], d["m"]), gwant, "group host affine", names)
    assert gwant[0][gx.derived.row(10, 2)] == 3


def test_argument_errors(eng):
    import torch
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    x = xc.ExtCase(mc.valid_transcripts([2, 3], seed=921, threads=THREADS), seed=922)
    a = x.args()
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    outs = [np.zeros(x.n, np.uint8), np.zeros(x.T, np.uint8), np.zeros((x.T, 64), np.uint8), np.zeros((x.T, 32), np.uint8), np.zeros((x.T, 64), np.uint8)]
    call = lambda fmt, cols, T=x.T: lib.jjs_multisig_combine(fmt, *cols, p(a[5]), T, *[p(v) for v in outs])  # noqa: E731
    cols = [p(c) for c in a[:5]]
    assert call(1, cols) == 0
    assert call(2, cols) == -1 and call(3, cols) == -1 and call(-1, cols) == -1, "wire is not part of the multisignature calls"
    assert call(2, cols, T=0) == -1 and call(1, cols, T=0) == 0
    for k in range(5):
        assert call(1, cols[:k] + [None] + cols[k + 1:]) == -1, k
    ins = [dev(c) for c in a[:5]]
    douts = [dev(v) for v in outs]
    q = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in range(1, 4):
        din = [q(t) for t in ins]
        din[k] = None
        assert lib.jjs_multisig_combine_ext_dev(*din, p(a[5]), x.T, *[q(t) for t in douts], s) == -1, k
        din[k] = ctypes.c_void_p(ins[k].data_ptr() + 8)
        assert lib.jjs_multisig_combine_ext_dev(*din, p(a[5]), x.T, *[q(t) for t in douts], s) == -1, ("misaligned", k)
    # the group: a stale handle, and n B >= 2^32 -- refused by arithmetic, no column is that long
    _, pk_ext = group_case(8)
    g = eng.multisig_group(pk_ext, fmt="ext")
    h = g.handle
    gz, gm = dev(np.zeros((8, 32), np.uint8)), dev(np.zeros((1, 32), np.uint8))
    gr = dev(np.zeros((8, 96), np.uint8))
    gout = [dev(np.zeros(8, np.uint8)), dev(np.zeros(1, np.uint8)), dev(np.zeros((1, 32), np.uint8)), dev(np.zeros((1, 64), np.uint8))]
    dargs = lambda B: (q(gz), q(gr), q(gr), q(gm), B, *[q(t) for t in gout], s)  # noqa: E731
    hz, hr, hm = np.zeros((8, 32), np.uint8), np.zeros((8, 96), np.uint8), np.zeros((1, 32), np.uint8)
    hout = [np.zeros(8, np.uint8), np.zeros(1, np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)]
    hargs = lambda B: (p(hz), p(hr), p(hr), p(hm), B, *[p(v) for v in hout])  # noqa: E731
    assert lib.jjs_msig_group_combine_ext_dev(h, *dargs(1)) == 0 and lib.jjs_msig_group_combine(h, 1, *hargs(1)) == 0
    torch.cuda.synchronize()
    assert hout[0].tolist() == [3] * 8, "Z = 0 everywhere: status 3, not InvalidPoint"
    assert (1 << 29) * 8 == 1 << 32
    assert lib.jjs_msig_group_combine_ext_dev(h, *dargs(1 << 29)) == -1 and lib.jjs_msig_group_combine(h, 1, *hargs(1 << 29)) == -1
    assert lib.jjs_msig_group_combine(h, 2, *hargs(1)) == -1
    g.close()
    assert lib.jjs_msig_group_combine_ext_dev(h, *dargs(1)) == -1 and lib.jjs_msig_group_combine(h, 1, *hargs(1)) == -1
    assert lib.jjs_msig_group_combine(h, 1, *hargs(0)) == -1, "a stale handle is refused before the empty call returns"
    torch.cuda.synchronize()

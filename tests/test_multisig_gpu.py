"""jjs_multisig_combine_dev on the device in every mode it runs in, against jjs_oracle_c.multisig_combine on 16 threads
(cases and expected values: multisig_cases.py, which the CPU build runs as well in test_multisig_host.py).

The launch code picks, per pass, one lane per item or eight cooperating lanes per item for the hash passes (1: per share;
2 and 4: per transcript) by `count <= 8192`.  The calls below reach all four combinations, both sides of 8192 for shares and
for transcripts, 256 beside 257 participants in both modes, and a call with more shares than msig_kernel has resident lanes
(second trip of its grid-stride loop).  Every call prints n, T, the lanes of passes 1 / 2 / 4 and the number of shares left
uncompared (beside a coordinate >= q only; multisig_cases.check caps them under 2 % of the call).

  call  shares        transcripts         pass 1   passes 2, 4
  A     8192          < 8192              8 lanes  8 lanes      every call is built of distinct transcripts
  B     8193          < 8192              1 lane   8 lanes      A and one more transcript
  C     > 8192        8192 / 8193         1 lane   8 / 1 lanes  the same shares: the second has one empty transcript more
  D     8192          8193, many empty    8 lanes  1 lane
  E     > 8192        > 8192              1 lane   1 lane       C with transcripts of 256, 257 and 601 participants in the middle
  F     513           2                   8 lanes  8 lanes      256 and 257 participants alone
  G     > 1.25 x resident lanes           1 lane   1 lane       distinct while the oracle takes under a minute, else tiled
"""
import ctypes
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import multisig_cases as mc
from helpers import ARG_ORDER, make_batch, oracle_verify

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = 16


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(eng, case):
    a = case.args()
    return tuple(t.cpu().numpy() for t in eng.multisig_combine(*[dev(x) for x in a[:5]], a[5]))


def run_and_check(eng, name, case, e, modes, note=""):
    assert mc.lane_modes(case.n, case.T) == modes, (name, case.n, case.T)
    t0 = time.time()
    got = run(eng, case)
    dt = time.time() - t0
    uncompared = mc.check(case, e, got, name)
    print(f"multisig call {name}: n={case.n} T={case.T} lanes pass 1/2/4 = {modes[0]}/{modes[1]}/{modes[2]} "
          f"uncompared={uncompared} ({100.0 * uncompared / case.n:.2f} %) device+copies {dt * 1e3:.0f} ms {note}")
    return got


def same_outputs(a, b, label):
    for k, x, y in zip(mc.OUTPUTS, a, b):
        assert x.shape == y.shape and (x == y).all(), (label, k)


# ---- the calls (built once per module run; B reuses A, E reuses C and F) ----
@functools.lru_cache(None)
def call_A():
    case, sections = mc.mixed_call(8192, seed=10, threads=THREADS)
    assert case.T <= mc.COOP_MAX_ITEMS and mc.straddles(case, 32) and mc.straddles(case, 256)
    return case, sections, mc.expected(case, THREADS)


@functools.lru_cache(None)
def call_C():
    """8192 transcripts of 1 to 3 participants with the special transcripts among them (more than 8192 shares), and the same
    shares as 8193 transcripts: one empty transcript more."""
    rng = np.random.default_rng(20)
    sp = mc.specials(20, THREADS)
    fill = mc.valid_transcripts(rng.choice([1, 2, 3], mc.COOP_MAX_ITEMS - sp.T, p=[0.55, 0.35, 0.10]), 21, threads=THREADS)
    for t in range(3, fill.T, 7):
        fill.corrupt(t, int(rng.integers(0, fill.sizes()[t])))
    cut = 4001
    c2 = mc.concat(fill.slice(0, cut), sp, fill.slice(cut, fill.T))
    c1 = mc.concat(c2.slice(0, 6000), mc.valid_transcripts([0], 22), c2.slice(6000, c2.T))
    assert c2.T == mc.COOP_MAX_ITEMS and c1.T == c2.T + 1 and c1.n == c2.n > mc.COOP_MAX_ITEMS
    assert mc.straddles(c2, 32) and mc.straddles(c2, 256)
    return c2, c1


@functools.lru_cache(None)
def long_pair():
    return mc.valid_transcripts([mc.TABLE_PARTICIPANTS, mc.TABLE_PARTICIPANTS + 1], seed=40, threads=THREADS)


# ---- modes and boundaries ----
def test_resident_lanes_are_reported(eng):
    from jubjub_schnorr_amd import _ffi
    lanes = _ffi.lib().jjs_debug_msig_resident_lanes()
    print(f"msig_kernel resident lanes on this device: {lanes}")
    assert lanes > 0 and lanes % 256 == 0


def test_call_A_and_B_either_side_of_8192_shares(eng):
    case, sections, e = call_A()
    got_a = run_and_check(eng, "A", case, e, (8, 8, 8))
    mc.check_sections(case, sections, got_a, "A")
    one_more = mc.valid_transcripts([1], seed=11, threads=THREADS)
    b = mc.concat(case, one_more)
    assert b.n == mc.COOP_MAX_ITEMS + 1
    got_b = run_and_check(eng, "B", b, mc.expected(b, THREADS), (1, 8, 8))
    mc.check_sections(b, sections, got_b, "B")
    # the shared transcripts: identical bytes from pass 1 on eight lanes and on one
    same_outputs(got_a, (got_b[0][:case.n],) + tuple(x[:case.T] for x in got_b[1:]), "A in B")


def test_call_C_either_side_of_8192_transcripts(eng):
    c2, c1 = call_C()
    got2 = run_and_check(eng, "C (T=8192)", c2, mc.expected(c2, THREADS), (1, 8, 8))
    got1 = run_and_check(eng, "C (T=8193)", c1, mc.expected(c1, THREADS), (1, 1, 1))
    keep = c1.sizes() != 0
    assert (~keep).sum() == 1 and got1[4][~keep].tolist() == [5]
    same_outputs(got2, (got1[0],) + tuple(x[keep] for x in got1[1:]), "C: the two differ only in mode")


def test_call_D_many_empty_transcripts(eng):
    case, sections = mc.mixed_call(mc.COOP_MAX_ITEMS, seed=30, T=mc.COOP_MAX_ITEMS + 1, threads=THREADS, top=6)
    empty = case.sizes() == 0
    assert empty[[0, 1, -2, -1]].all() and empty.sum() > 5000 and (~empty[:-1] & empty[1:]).any()
    got = run_and_check(eng, "D", case, mc.expected(case, THREADS), (8, 1, 1))
    mc.check_sections(case, sections, got, "D")       # status 5 and all-zero outputs for exactly the empty transcripts


def test_call_E_long_transcripts_on_single_lanes_and_F_alone(eng):
    c2, c1 = call_C()
    pair = long_pair()
    got_f = run_and_check(eng, "F", pair, mc.expected(pair, THREADS), (8, 8, 8), "256 and 257 participants alone")
    assert got_f[4].tolist() == [0, 0]
    long3 = mc.valid_transcripts([601], seed=41, threads=THREADS)
    long3.corrupt(0, 300)
    at, at3 = 1001, 5000 + pair.T
    e_case = mc.concat(c1.slice(0, at), pair, c1.slice(at, 5000), long3, c1.slice(5000, c1.T))
    assert e_case.sizes()[[at, at + 1, at3]].tolist() == [256, 257, 601]
    got_e = run_and_check(eng, "E", e_case, mc.expected(e_case, THREADS), (1, 1, 1), f"256, 257 at transcripts {at}, {at + 1}; 601 at {at3}")
    lo = int(e_case.offsets[at])
    same_outputs(got_f, (got_e[0][lo:lo + pair.n],) + tuple(x[at:at + 2] for x in got_e[1:]), "F inside E")
    assert got_e[4][at3] == 4 and got_e[1][at3].any() and not got_e[2][at3].any()


def test_call_G_more_shares_than_resident_lanes(eng):
    """More shares than msig_kernel has resident lanes (grid_msig * BLOCK, read from the engine): the grid-stride loop takes a
    second trip and a lane's workspace is used again.  The size is the next odd multiple of a base above 1.25 times that number;
    the base has an odd transcript count and an odd share count.  DISTINCT transcripts throughout while the oracle's work for
    the call stays under about a minute (14 k shares/s on 16 threads, README); beyond, TILED: copies of the base, the whole
    base against the oracle and every copy against the first, byte for byte -- an index off by the grid's stride or by a
    power of two then lands on other data, not on a replica.  The printed line says which of the two was done."""
    from jubjub_schnorr_amd import _ffi
    lanes = _ffi.lib().jjs_debug_msig_resident_lanes()
    assert lanes > 0
    base, sections = mc.mixed_call(3999, seed=50, threads=THREADS)
    if base.T % 2 == 0:
        base = mc.concat(base, mc.valid_transcripts([2], seed=51, threads=THREADS))
    assert base.T % 2 == 1 and base.n % 2 == 1
    reps = int(1.25 * lanes) // base.n + 1
    reps += 1 - reps % 2
    n = reps * base.n
    assert reps % 2 == 1 and n > 1.25 * lanes
    if n / 14000.0 <= 60.0:
        case, sections = mc.mixed_call(n, seed=52, threads=THREADS)
        got = run_and_check(eng, "G", case, mc.expected(case, THREADS), (1, 1, 1), f"DISTINCT transcripts; resident lanes {lanes}")
        mc.check_sections(case, sections, got, "G")
        return
    case, e = mc.tile(base, reps), mc.tile_expected(mc.expected(base, THREADS), reps, base.T)
    got = run_and_check(eng, "G", case, e, (1, 1, 1), f"TILED: {reps} copies of n={base.n} T={base.T}; resident lanes {lanes}")
    mc.check_sections(base, sections, tuple(x[:base.n if k == 0 else base.T] for k, x in enumerate(got)), "G")
    for k, x in enumerate(got):
        per = base.n if k == 0 else base.T
        assert (x.reshape(reps, per, -1) == x[:per].reshape(1, per, -1)).all(), mc.OUTPUTS[k]


# ---- state across calls ----
def test_scratch_reuse_across_calls(eng, tmp_path):
    """multisig_state_child.py runs small, grow, small, long_at_3, long_at_5, long_at_3 on a fresh engine; here the same calls run
    in another order on this module's engine, whatever it ran before: identical bytes, and the oracle's."""
    out = str(tmp_path / "state.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "multisig_state_child.py"), out], capture_output=True, text=True, timeout=420)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]
    alone = np.load(out)
    calls = mc.state_calls(THREADS)
    for name in ("long_at_5", "grow", "long_at_3", "small", "long_at_5"):
        got = run_and_check(eng, f"state/{name}", calls[name], mc.expected(calls[name], THREADS), mc.lane_modes(calls[name].n, calls[name].T))
        same_outputs(tuple(alone[f"{name}.{k}"] for k in mc.OUTPUTS), got, name)


def test_call_on_a_second_stream_beside_a_verify(eng):
    import torch
    case, _, e = call_A()
    base = run(eng, case)
    a = case.args()
    d_args = [dev(x) for x in a[:5]]
    b = make_batch("single", 4096, seed=5, n_keys=64)
    v_args = [dev(b[k]) for k in ARG_ORDER["single"]]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        out = eng.multisig_combine(*d_args, a[5])
    with torch.cuda.stream(s2):
        st, tally = eng.verify("single", *v_args)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in out)
    same_outputs(base, got, "second stream")
    mc.check(case, e, got, "second stream")
    assert st.cpu().numpy().tolist() == oracle_verify("single", b, threads=THREADS).tolist()


# ---- the ABI itself ----
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _abi_call(lib, case, fill, with_status=True):
    import torch
    a = case.args()
    ins = [dev(x) for x in a[:5]]
    full = lambda *shape: torch.full(shape, fill, dtype=torch.uint8, device="cuda")  # noqa: E731
    st, ts, agg, su, sr = full(case.n), full(case.T), full(case.T, 64), full(case.T, 32), full(case.T, 64)
    rc = lib.jjs_multisig_combine_dev(*[_ptr(x) for x in ins], a[5].ctypes.data_as(ctypes.c_void_p), case.T, _ptr(st),
                                      _ptr(ts) if with_status else None, _ptr(agg), _ptr(su), _ptr(sr),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, tuple(x.cpu().numpy() for x in (st, agg, su, sr, ts))


def test_every_output_byte_is_written(eng):
    """Engine.multisig_combine hands torch.empty buffers to the ABI: the zeros of an empty or failed transcript must be written,
    not left over.  Two prefills, 0xA5 and 0x5A, give the same bytes, and the oracle's; transcript_status = NULL changes nothing else."""
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    case, sections = mc.mixed_call(2201, seed=3, T=900, threads=THREADS, top=6)
    e = mc.expected(case, THREADS)
    rc1, got1 = _abi_call(lib, case, 0xA5)
    rc2, got2 = _abi_call(lib, case, 0x5A)
    assert rc1 == 0 and rc2 == 0
    same_outputs(got1, got2, "prefill")
    mc.check(case, e, got1, "prefill 0xA5")
    mc.check_sections(case, sections, got1, "prefill 0xA5")
    rc3, got3 = _abi_call(lib, case, 0xA5, with_status=False)
    assert rc3 == 0
    same_outputs(got1[:4], got3[:4], "transcript_status = NULL")
    assert (got3[4] == 0xA5).all()
    mc.check(case, e, got3[:4] + (None,), "transcript_status = NULL")


def test_argument_errors_launch_nothing(eng):
    """The checks the entry point makes before any launch: JJS_ERR_ARG, outputs untouched.  (Only what it checks: nothing here
    is outside the ABI's contract in a way the entry point does not see.)"""
    import torch
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    case = mc.valid_transcripts([2, 1], seed=70, threads=THREADS)
    ins = [dev(x) for x in case.args()[:5]]
    full = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    outs = [full(16), full(16), full(16, 64), full(16, 32), full(16, 64)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(offsets, T, z=ins[0], m=ins[4]):
        offs = np.asarray(offsets, np.uint32)
        return lib.jjs_multisig_combine_dev(_ptr(z), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]), _ptr(m), offs.ctypes.data_as(ctypes.c_void_p), T,
                                            *[_ptr(x) for x in outs], stream)
    limit = 1 << 24                                             # csrc/device_kernels.h JJS_MSIG_PARTICIPANTS_LIMIT
    errors = {"offsets[0] != 0": ([1, 3], 1), "decreasing offsets": ([0, 3, 2], 2), "count above the limit": ([0, limit + 1], 1),
              "null z with n > 0": ([0, 2, 3], 2, None), "null m": ([0, 2, 3], 2, ins[0], None)}
    for what, a in errors.items():
        assert call(*a) == -1, what                             # JJS_ERR_ARG
        assert lib.jjs_last_error(), what
    assert call([0, 2, 3], 0) == 0                              # n_transcripts = 0: JJS_OK, nothing to do
    torch.cuda.synchronize()
    for x in outs:
        assert (x.cpu().numpy() == 0xA5).all()
    assert call([0, 2, 3], 2) == 0                              # and the same arguments without the error are a good call
    torch.cuda.synchronize()
    assert outs[1].cpu().numpy()[:2].tolist() == [0, 0]

"""jjs_msig_group_* on the device: the cases of test_msig_group_host.py through the C ABI, against jjs_oracle_c.multisig_combine
on the tiled inline form (msig_group_cases.py) AND, byte for byte, against jjs_multisig_combine_dev on that form in the same
process.  The hash passes take eight lanes per transcript up to 8192 transcripts and one beyond: a call on either side; one
call has more shares than the multisignature kernels have resident lanes (second trip of the grid-stride loops; tiled copies
of a base call, as test_multisig_gpu.py's call G).  Then two groups on two streams beside a verify, lifetime, arguments.
Every call prints its size and what it left uncompared (shares beside a coordinate >= q only)."""
import ctypes
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import jjs_oracle as o
import msig_group_cases as gcs
import multisig_cases as mc
from helpers import ARG_ORDER, make_batch, oracle_verify

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = 16
OUT = ("share_status", "sig_u", "sig_R", "transcript_status")


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def create(lib, PK):
    PK = np.ascontiguousarray(PK, np.uint8)
    h = ctypes.c_uint64(0)
    rc = lib.jjs_msig_group_create(PK.ctypes.data_as(ctypes.c_void_p) if len(PK) else None, len(PK), ctypes.byref(h))
    return rc, h.value


def aggregate(lib, h):
    out = np.zeros(64, np.uint8)
    assert lib.jjs_msig_group_aggregate_pk(h, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def abi_call(lib, h, gc, fill=0xA5, with_status=True, stream=None, ins=None):
    """One jjs_msig_group_combine_dev on prefilled outputs.  Returns rc and (share_status, sig_u, sig_R, transcript_status)."""
    import torch
    ins = ins or [dev(x) for x in gc.call_args()]
    full = lambda *shape: torch.full(shape, fill, dtype=torch.uint8, device="cuda")  # noqa: E731
    st, ts, su, sr = full(gc.case.n), full(gc.T), full(gc.T, 32), full(gc.T, 64)
    s = stream or torch.cuda.current_stream()
    rc = lib.jjs_msig_group_combine_dev(h, *[_ptr(x) for x in ins], gc.T, _ptr(st), _ptr(ts) if with_status else None, _ptr(su), _ptr(sr),
                                        ctypes.c_void_p(s.cuda_stream))
    return rc, (st, su, sr, ts)


def host(outs):
    import torch
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in outs)


def inline(eng, gc):
    a = gc.case.args()
    st, agg, su, sr, ts = (t.cpu().numpy() for t in eng.multisig_combine(*[dev(x) for x in a[:5]], a[5]))
    return (st, su, sr, ts), agg


def same(a, b, label):
    for k, x, y in zip(OUT, a, b):
        assert x.shape == y.shape and (x == y).all(), (label, k, np.nonzero((x != y).reshape(len(x), -1).any(1))[0][:8].tolist())


def run_and_check(eng, lib, gc, label, e=None, h=None):
    """The group call against the oracle and against the inline call; returns the group call's outputs."""
    own = h is None
    if own:
        rc, h = create(lib, gc.PK)
        assert rc == 0 and h != 0, label
    t0 = time.time()
    rc, outs = abi_call(lib, h, gc)
    assert rc == 0, (label, lib.jjs_last_error())
    got = host(outs)
    dt = time.time() - t0
    agg = aggregate(lib, h)
    e = e or mc.expected(gc.case, THREADS)
    uncompared = mc.check(gc.case, e, gcs.as_inline_outputs(gc, agg, got), label)
    want, want_agg = inline(eng, gc)
    same(want, got, label + ": group call against inline call")
    cmp = e.cmp_agg
    assert (want_agg[cmp] == agg[None]).all(), (label, "aggregate key against the inline call's rows")
    print(f"group call {label}: n={gc.n} T={gc.T} shares={gc.case.n} hash lanes={8 if gc.T <= mc.COOP_MAX_ITEMS else 1} "
          f"uncompared={uncompared} device+copies {dt * 1e3:.0f} ms")
    if own:
        assert lib.jjs_msig_group_destroy(h) == 0
    return got


@functools.lru_cache(None)
def group8():
    """The 8-participant group's two calls: the mix in 40 transcripts, and 64 transcripts with a coordinate >= q."""
    gc = gcs.group_transcripts(8, 104, seed=200, threads=THREADS)
    a, b = gc.slice(0, 40), gc.slice(40, 104)
    gcs.mix(a)
    b.case.bad_coord(31, 0, "R", 1, o.Q)
    return a, b


# ---- the cases of the CPU build ----
@pytest.mark.parametrize("n,T", [(1, 12), (2, 40)])
def test_mix_of_transcripts(eng, n, T):
    from jubjub_schnorr_amd import _ffi
    gc = gcs.group_transcripts(n, T, seed=100 + n, threads=THREADS)
    gcs.mix(gc, {1: [("R", 0, o.Q), ("S", 1, gcs.ALL_ONES)], 2: [("S", 0, o.Q)]}[n])
    run_and_check(eng, _ffi.lib(), gc, f"mix n={n}")


def test_eight_participants_mix_and_coordinate(eng):
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    a, b = group8()
    rc, h = create(lib, a.PK)
    assert rc == 0
    got = run_and_check(eng, lib, a, "mix n=8", h=h)
    assert got[3][:9].tolist() == [0, 4, 4, 4, 4, 3, 4, 3, 3] and (got[3][9:] == 0).all()
    got = run_and_check(eng, lib, b, "coordinate n=8", h=h)
    assert got[0][31 * 8] == 3 and got[3][31] == 3
    info = (ctypes.c_uint64 * 4)()
    assert lib.jjs_msig_group_info(h, info) == 0
    assert list(info)[:2] == [8, 6] and info[2] >= 8 * 43 * 33 * 144 and info[3] == 2
    assert lib.jjs_msig_group_destroy(h) == 0


@pytest.mark.parametrize("n", [mc.TABLE_PARTICIPANTS, mc.TABLE_PARTICIPANTS + 1])
def test_last_table_tag_and_first_computed_tag(eng, n):
    from jubjub_schnorr_amd import _ffi
    gc = gcs.group_transcripts(n, 3, seed=130 + n, threads=THREADS)
    gc.case.corrupt(1, n - 1)
    gc.case.bad_z(2, n // 2, o.R_ORDER)
    got = run_and_check(eng, _ffi.lib(), gc, f"n={n}")
    assert got[3].tolist() == [0, 4, 3]


def test_identity_repeated_and_small_order_keys(eng):
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    gc = gcs.group_transcripts(5, 6, seed=140, zero_sk=(1,), same_sk=((3, 0),), threads=THREADS)
    gc.case.corrupt(4, 3)
    assert run_and_check(eng, lib, gc, "identity and repeated keys")[3].tolist() == [0, 0, 0, 0, 4, 0]
    # a key with a small-order part under shares the reference accepts (msig_group_cases.torsion_key_case)
    tk = gcs.torsion_key_case()
    assert run_and_check(eng, lib, tk, "key with a small-order part")[3].tolist() == [0] * tk.T
    base = gcs.group_transcripts(4, 5, seed=150, threads=THREADS)
    base.case.corrupt(2, 1)
    for name, point in mc.small_order_points():
        for j in (0, 3):
            run_and_check(eng, lib, gcs.with_point(base, j, point), f"{name} as key {j}")


# ---- lane modes and the grid-stride loop ----
def test_more_than_8192_transcripts_take_one_hash_lane(eng):
    """8193 transcripts of two participants (one lane per transcript in the hash passes, and the share pass by participant),
    with the mix and one coordinate >= q among them; the first 8192 of them alone run on eight lanes and give the same bytes."""
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    gc = gcs.group_transcripts(2, mc.COOP_MAX_ITEMS + 1, seed=210, threads=THREADS)
    gcs.mix(gc, [("R", 1, o.Q)])
    for t in range(50, gc.T, 97):
        gc.case.corrupt(t, t % 2)
    rc, h = create(lib, gc.PK)
    assert rc == 0
    e = mc.expected(gc.case, THREADS)
    one = run_and_check(eng, lib, gc, "8193 transcripts", e=e, h=h)
    part = gc.slice(0, mc.COOP_MAX_ITEMS)
    eight = run_and_check(eng, lib, part, "8192 transcripts", h=h)
    same(eight, (one[0][:part.case.n],) + tuple(x[:part.T] for x in one[1:]), "the two differ only in lane mode")
    assert lib.jjs_msig_group_destroy(h) == 0


def test_more_shares_than_resident_lanes(eng):
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    lanes = lib.jjs_debug_msig_resident_lanes()
    assert lanes > 0
    _, base = group8()
    reps = int(1.25 * lanes) // base.case.n + 1
    reps += 1 - reps % 2
    gc = base.tile(reps)
    assert gc.case.n > 1.25 * lanes
    e = mc.tile_expected(mc.expected(base.case, THREADS), reps, base.T)
    got = run_and_check(eng, lib, gc, f"{reps} copies of T={base.T} (resident lanes {lanes})", e=e)
    for k, x in enumerate(got):
        per = base.case.n if k == 0 else base.T
        assert (x.reshape(reps, per, -1) == x[:per].reshape(1, per, -1)).all(), OUT[k]


# ---- streams, lifetime, arguments ----
def test_two_groups_on_two_streams_beside_a_verify(eng):
    import torch
    a, _ = group8()
    b = gcs.group_transcripts(3, 50, seed=220, threads=THREADS)
    b.case.corrupt(7, 2)
    ea, eb = mc.expected(a.case, THREADS), mc.expected(b.case, THREADS)
    batch = make_batch("single", 4096, seed=5, n_keys=64)
    v_args = [dev(batch[k]) for k in ARG_ORDER["single"]]
    with eng.multisig_group(a.PK) as ga, eng.multisig_group(b.PK) as gb:
        ins_a, ins_b = [dev(x) for x in a.call_args()], [dev(x) for x in b.call_args()]
        s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = []
        for turn in range(3):
            with torch.cuda.stream(s1 if turn % 2 == 0 else s2):
                outs.append(("a", ga.combine(*ins_a)))
            with torch.cuda.stream(s2 if turn % 2 == 0 else s1):
                outs.append(("b", gb.combine(*ins_b)))
            if turn == 1:
                with torch.cuda.stream(s3):
                    st, tally = eng.verify("single", *v_args)
        torch.cuda.synchronize()
        for which, out in outs:
            gc, e, grp = (a, ea, ga) if which == "a" else (b, eb, gb)
            st_, su, sr, ts = (x.cpu().numpy() for x in out)
            mc.check(gc.case, e, gcs.as_inline_outputs(gc, grp.aggregate_pk, (st_, su, sr, ts)), f"stream turn {which}")
        assert st.cpu().numpy().tolist() == oracle_verify("single", batch, threads=THREADS).tolist()
        assert ga.info()["calls"] == 3 and gb.info()["participants"] == 3


def test_destroy_trim_and_stale_handles(eng):
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    a, _ = group8()
    e = mc.expected(a.case, THREADS)
    rc, h = create(lib, a.PK)
    rc2, h2 = create(lib, a.PK[:3])
    assert rc == 0 and rc2 == 0 and h != h2 and h and h2
    assert lib.jjs_msig_group_destroy(h2) == 0
    assert lib.jjs_trim() == 0                                   # frees the destroyed group only
    rc, outs = abi_call(lib, h, a)
    assert rc == 0
    mc.check(a.case, e, gcs.as_inline_outputs(a, aggregate(lib, h), host(outs)), "after jjs_trim")
    # a queued call still reads the group's memory after destroy
    agg = aggregate(lib, h)
    rc, outs = abi_call(lib, h, a, fill=0x5A)
    assert rc == 0 and lib.jjs_msig_group_destroy(h) == 0
    mc.check(a.case, e, gcs.as_inline_outputs(a, agg, host(outs)), "queued before destroy")
    info = (ctypes.c_uint64 * 4)()
    out64 = np.zeros(64, np.uint8)
    for stale in (h, h2, 0, 12345):
        assert abi_call(lib, stale, a)[0] == -1, stale
        assert lib.jjs_msig_group_destroy(stale) == -1 and lib.jjs_msig_group_info(stale, info) == -1
        assert lib.jjs_msig_group_aggregate_pk(stale, out64.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.jjs_trim() == 0


def test_handles_of_one_kind_are_unknown_to_the_other(eng):
    """Key sets and signer groups share one registry type and one generation counter: a live handle of either kind is an
    unknown handle to every entry point of the other (JJS_ERR_ARG, nothing destroyed, nothing launched), also after one
    kind's index has been freed and the other kind has registered again.  Two keys, two participants, one item, one transcript."""
    import torch
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    b = make_batch("single", 2, seed=77, n_keys=2, mix=False)
    ks = eng.keyset("single", b["PK"])
    assert ks.key_status.tolist() == [0, 0]
    gc = gcs.group_transcripts(2, 1, seed=230, threads=THREADS)
    rc, grp = create(lib, gc.PK)
    assert rc == 0 and grp and ks.handle and grp != ks.handle
    kd = [dev(x) for x in (np.zeros(1, np.int32), b["u"][:1], b["R"][:1], b["m"][:1])]           # key_idx, u, R, m
    gd = [dev(x) for x in gc.call_args()]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    info = (ctypes.c_uint64 * 8)()
    out64 = np.zeros(64, np.uint8)

    def keyset_calls(h):
        """rc of jjs_keyset_info, _verify_dev, _verify_all_dev on handle h, and what the two calls wrote (prefilled 0xA5)."""
        st = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
        tally = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        verdict = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rcs = [lib.jjs_keyset_info(h, info),
               lib.jjs_keyset_verify_dev(h, 0, _ptr(kd[0]), _ptr(kd[1]), _ptr(kd[2]), None, _ptr(kd[3]), 1, _ptr(st), _ptr(tally), stream),
               lib.jjs_keyset_verify_all_dev(h, 0, _ptr(kd[0]), _ptr(kd[1]), _ptr(kd[2]), None, _ptr(kd[3]), 1, _ptr(verdict), stream)]
        torch.cuda.synchronize()
        return rcs, (st.cpu().numpy().tobytes(), tally.cpu().numpy().tobytes(), verdict.cpu().numpy().tobytes())

    def group_calls(h):
        """rc of jjs_msig_group_info, _aggregate_pk, _combine_dev on handle h, and what they wrote (prefilled 0xA5)."""
        out64[:] = 0xA5
        rcs = [lib.jjs_msig_group_info(h, info), lib.jjs_msig_group_aggregate_pk(h, out64.ctypes.data_as(ctypes.c_void_p))]
        rc, outs = abi_call(lib, h, gc, ins=gd)
        return rcs + [rc], (out64.tobytes(),) + tuple(x.tobytes() for x in host(outs))

    untouched_k = (b"\xa5" * 16, b"\xff" * 32, b"\x5a" * 4)
    untouched_g = (b"\xa5" * 64, b"\xa5" * 2, b"\xa5" * 32, b"\xa5" * 64, b"\xa5")
    rcs, first_k = keyset_calls(ks.handle)
    assert rcs == [0, 0, 0]
    assert first_k[0][0] == oracle_verify("single", b, threads=THREADS)[0] == 0
    assert first_k[1] == np.array([1, 0, 0, 0], np.int64).tobytes() and first_k[2] == np.array([1], np.int32).tobytes()
    got = run_and_check(eng, lib, gc, "one transcript of two", h=grp)
    rcs, first_g = group_calls(grp)
    assert rcs == [0, 0, 0] and first_g == (aggregate(lib, grp).tobytes(),) + tuple(x.tobytes() for x in got)

    # the live key set is no signer group, the live signer group is no key set
    assert group_calls(ks.handle) == ([-1, -1, -1], untouched_g) and lib.jjs_msig_group_destroy(ks.handle) == -1
    assert keyset_calls(grp) == ([-1, -1, -1], untouched_k) and lib.jjs_keyset_destroy(grp) == -1
    assert b"key set" in lib.jjs_last_error()
    assert keyset_calls(ks.handle) == ([0, 0, 0], first_k) and group_calls(grp) == ([0, 0, 0], first_g)

    # the key set's index is free again; the next signer group takes an index of its own registry and a new generation
    old = ks.handle
    assert lib.jjs_keyset_destroy(old) == 0
    ks.handle = 0
    rc, grp2 = create(lib, gc.PK)
    assert rc == 0 and grp2 and grp2 not in (old, grp)
    assert keyset_calls(old) == ([-1, -1, -1], untouched_k) and lib.jjs_keyset_destroy(old) == -1
    assert group_calls(old) == ([-1, -1, -1], untouched_g) and lib.jjs_msig_group_destroy(old) == -1
    assert keyset_calls(grp2) == ([-1, -1, -1], untouched_k) and lib.jjs_keyset_destroy(grp2) == -1
    assert group_calls(grp) == ([0, 0, 0], first_g) and group_calls(grp2) == ([0, 0, 0], first_g)
    assert lib.jjs_trim() == 0
    assert group_calls(grp) == ([0, 0, 0], first_g) and group_calls(grp2) == ([0, 0, 0], first_g)
    assert lib.jjs_msig_group_destroy(grp) == 0 and lib.jjs_msig_group_destroy(grp2) == 0


def test_state_across_shutdown_in_a_fresh_process():
    p = subprocess.run([sys.executable, os.path.join(HERE, "msig_group_state_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]


def test_arguments_null_status_and_prefilled_outputs(eng):
    import torch
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    a, _ = group8()
    e = mc.expected(a.case, THREADS)
    # registration
    assert create(lib, np.zeros((0, 64), np.uint8))[0] == -1
    bad = a.PK.copy()
    bad[5, 32:] = mc._fe([o.Q])[0]
    assert create(lib, bad)[0] == -1 and lib.jjs_last_error()
    assert lib.jjs_msig_group_create(a.PK.ctypes.data_as(ctypes.c_void_p), 8, None) == -1
    rc, h = create(lib, a.PK)
    assert rc == 0
    agg = aggregate(lib, h)
    # two prefills give the same bytes; transcript_status = NULL changes nothing else
    rc1, o1 = abi_call(lib, h, a, fill=0xA5)
    rc2, o2 = abi_call(lib, h, a, fill=0x5A)
    rc3, o3 = abi_call(lib, h, a, fill=0xA5, with_status=False)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    g1, g2, g3 = host(o1), host(o2), host(o3)
    same(g1, g2, "prefill")
    mc.check(a.case, e, gcs.as_inline_outputs(a, agg, g1), "prefill 0xA5")
    same(g1[:3], g3[:3], "transcript_status = NULL")
    assert (g3[3] == 0xA5).all()
    # argument errors launch nothing
    ins = [dev(x) for x in a.call_args()]
    full = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    outs = [full(a.case.n), full(a.T), full(a.T, 32), full(a.T, 64)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(T, z=ins[0], m=ins[3], st=outs[0]):
        return lib.jjs_msig_group_combine_dev(h, _ptr(z), _ptr(ins[1]), _ptr(ins[2]), _ptr(m), T, _ptr(st), _ptr(outs[1]), _ptr(outs[2]),
                                              _ptr(outs[3]), stream)
    assert call(a.T, z=None) == -1 and call(a.T, m=None) == -1 and call(a.T, st=None) == -1
    assert call(1 << 29) == -1                                   # 2^29 transcripts of 8 participants: 2^32 shares
    assert call(0) == 0                                          # nothing to do, nothing written
    torch.cuda.synchronize()
    for x in outs:
        assert (x.cpu().numpy() == 0xA5).all()
    assert call(a.T) == 0
    torch.cuda.synchronize()
    assert (outs[1].cpu().numpy() == e.ts).all()
    assert lib.jjs_msig_group_destroy(h) == 0

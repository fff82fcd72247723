"""jjs_multisig_combine_keyset[_dev] on the device.  Every call is compared byte for byte with jjs_multisig_combine_dev (the
extended form: jjs_multisig_combine_ext_dev) on the gathered columns in the same process for the usable transcripts, and with
the fixed definition (every share 3, transcript 3, outputs zero) for the refused ones; the small calls with
jjs_oracle_c.multisig_combine as well (msig_keyset_cases.expected).  The set is the 16 keys of msig_keyset_cases.key_set."""
import ctypes
import functools

import numpy as np
import pytest

import jjs_oracle as o
import msig_group_cases as gcs
import msig_keyset_cases as kcs
import multisig_cases as mc
from helpers import to_pt

pytestmark = pytest.mark.gpu
THREADS = 16
FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


@functools.lru_cache(None)
def key_set():
    return kcs.key_set()


@pytest.fixture(scope="module")
def ks(eng):
    keys, _ = key_set()
    s = eng.keyset("single", keys)
    assert s.key_status.tolist() == kcs.KEY_STATUS
    assert s.info()["valid_keys"] == kcs.N_VALID
    yield s
    s.close()


def lib():
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _outputs(n, T, fill):
    import torch
    full = lambda *shape: torch.full(shape, fill, dtype=torch.uint8, device="cuda")  # noqa: E731
    return full(max(n, 1))[:n], full(T), full(T, 64), full(T, 32), full(T, 64)          # st, ts, agg, su, sr


def host(outs, with_status=True):
    import torch
    torch.cuda.synchronize()
    st, ts, agg, su, sr = (x.cpu().numpy() for x in outs)
    return st, agg, su, sr, (ts if with_status else None)


def keyset_call(h, kc, ext=False, fill=FILL, with_status=True):
    """One jjs_multisig_combine_keyset_dev on prefilled outputs: rc and the outputs in multisig_cases.check's order."""
    import torch
    idx, z, R, S, m, offs = kc.args()
    if ext:
        R, S = kc.R_ext if hasattr(kc, "R_ext") else kcs.to_ext(R), kcs.to_ext(S)
    ins = [dev(idx.view(np.int32)), dev(z), dev(R), dev(S), dev(m)]
    outs = _outputs(kc.case.n, kc.T, fill)
    st, ts, agg, su, sr = outs
    rc = lib().jjs_multisig_combine_keyset_dev(h, 1 if ext else 0, *[_ptr(x) for x in ins], offs.ctypes.data_as(ctypes.c_void_p), kc.T, _ptr(st),
                                               _ptr(ts) if with_status else None, _ptr(agg), _ptr(su), _ptr(sr),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        return rc, None
    got = host(outs, True)
    if not with_status:
        assert (got[4] == fill).all(), "transcript_status = NULL, and the buffer was written"
        got = got[:4] + (None,)
    return rc, got


def inline_call(kc, ext=False):
    import torch
    z, PK, R, S, m, offs = kc.inline_args()
    name = "jjs_multisig_combine_dev"
    if ext:
        PK, R, S = kcs.to_ext(PK), kc.R_ext if hasattr(kc, "R_ext") else kcs.to_ext(R), kcs.to_ext(S)
        name = "jjs_multisig_combine_ext_dev"
    ins = [dev(x) for x in (z, PK, R, S, m)]
    outs = _outputs(kc.case.n, kc.T, 0x5A)
    st, ts, agg, su, sr = outs
    rc = getattr(lib(), name)(*[_ptr(x) for x in ins], offs.ctypes.data_as(ctypes.c_void_p), kc.T, _ptr(st), _ptr(ts), _ptr(agg), _ptr(su),
                              _ptr(sr), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().jjs_last_error()
    return host(outs)


def written(got, label):
    for name, x in zip(mc.OUTPUTS, got):
        if x is not None and x.size:
            assert not (x.reshape(len(x), -1) == FILL).all(1).any(), (label, name, "a row was not written")


def run_and_check(h, kc, label, oracle=True, ext=False, with_status=True):
    rc, got = keyset_call(h, kc, ext=ext, with_status=with_status)
    assert rc == 0, (label, lib().jjs_last_error())
    written(got, label)
    kcs.check_against_inline(kc, got, inline_call(kc, ext=ext), label)
    if oracle:
        assert mc.check(kc.case, kcs.expected(kc, THREADS), got, label) == 0
    print(f"key-set call {label}: shares={kc.case.n} T={kc.T} refused={sorted(kc.refused)}")
    return got


@functools.lru_cache(None)
def call_a():
    """About 400 shares: ragged transcripts of 1-8 participants around the host harness's cases."""
    keys, sk = key_set()
    rng = np.random.default_rng(1000)
    fill = kcs.pool_transcripts(mc.ragged_sizes(rng, 340), 1001, keys, sk, threads=THREADS)
    for t in range(3, fill.T, 7):
        fill.case.corrupt(t, int(rng.integers(0, fill.case.sizes()[t])))
    mix, where = kcs.host_mix(keys, sk, threads=THREADS)
    cut = fill.T // 2
    head = kcs.KsCase(fill.case.slice(0, cut), fill.key_idx[:int(fill.case.offsets[cut])])
    tail = kcs.KsCase(fill.case.slice(cut, fill.T), fill.key_idx[int(fill.case.offsets[cut]):])
    return kcs.concat(head, mix, tail), {k: v + cut for k, v in where.items()}


# ---- (a) ----
def test_a_ragged_mix(ks):
    kc, where = call_a()
    assert 380 <= kc.case.n <= 420
    got = run_and_check(ks.handle, kc, "(a)")
    st, agg, su, sr, ts = got
    assert ts[where["empty"]] == 5 and ts[where["spoilt then z >= r"]] == 4 and ts[where["z >= r"]] == 3
    for what, _ in kcs.REFUSALS:
        assert ts[where[what]] == 3 and ts[where[what] - 1] == 0 and ts[where[what] + 1] == 0, what
    again = run_and_check(ks.handle, kc, "(a) transcript_status = NULL", oracle=False, with_status=False)
    for x, y in zip(got[:4], again[:4]):
        assert (x == y).all()


# ---- (b) ----
@functools.lru_cache(None)
def call_8193():
    keys, sk = key_set()
    rng = np.random.default_rng(1010)
    kc = kcs.pool_transcripts(mc.ragged_sizes(rng, mc.COOP_MAX_ITEMS + 1), 1011, keys, sk, threads=THREADS)
    assert kc.case.sizes()[-1] >= 1
    for t in range(5, kc.T, 11):
        kc.case.corrupt(t, 0)
    for k, (what, index) in enumerate(kcs.REFUSALS):
        kc.refuse(100 + 300 * k, 0, index, what)
    return kc


def test_b_both_hash_lane_modes_of_pass_1(ks):
    one = call_8193()
    assert one.case.n == mc.COOP_MAX_ITEMS + 1
    got1 = run_and_check(ks.handle, one, "(b) 8193 shares", oracle=False)
    # the same call without its last share (the last transcript loses it, or goes): 8192 shares, eight lanes per share
    c, last = one.case, one.T - 1
    if c.sizes()[last] == 1:
        eight = kcs.KsCase(c.slice(0, last), one.key_idx[:-1], one.refused)
    else:
        keys, sk = key_set()
        rng = np.random.default_rng(1012)
        eight = kcs.pool_transcripts(mc.ragged_sizes(rng, mc.COOP_MAX_ITEMS), 1013, keys, sk, threads=THREADS)
        eight.refuse(7, 0, 16, "index == n_keys")
    assert eight.case.n == mc.COOP_MAX_ITEMS
    run_and_check(ks.handle, eight, "(b) 8192 shares", oracle=False)
    assert got1[4][100] == 3


def test_b_8193_transcripts_most_of_them_empty(ks):
    keys, sk = key_set()
    rng = np.random.default_rng(1020)
    T = mc.COOP_MAX_ITEMS + 1
    kc = kcs.pool_transcripts(mc.empty_layout_sizes(rng, T, 300), 1021, keys, sk, threads=THREADS)
    full = np.nonzero(kc.case.sizes())[0]
    kc.case.corrupt(int(full[3]), 0)
    kc.refuse(int(full[5]), 0, kcs.IDENTITY_KEY, "identity")
    got = run_and_check(ks.handle, kc, "(b) 8193 transcripts")
    assert ((got[4] == 5) == (kc.case.sizes() == 0)).all() and got[4][full[5]] == 3 and got[4][full[3]] == 4


# ---- (c) ----
def test_c_257_participants_with_repetition(ks):
    keys, sk = key_set()
    kc = kcs.pool_transcripts([3, mc.TABLE_PARTICIPANTS + 1, 2, 1], 1030, keys, sk, threads=THREADS)
    kc.case.corrupt(1, 200)
    kc.refuse(2, 1, 0xFFFFFFFF, "index 0xFFFFFFFF")
    got = run_and_check(ks.handle, kc, "(c) long tags")
    assert got[4].tolist() == [0, 4, 3, 0] and got[0][3 + 200] == 4 and (np.delete(got[0][3:260], 200) == 0).all()


# ---- (d) ----
def test_d_extended_format(ks):
    kc, where = call_a()
    kc = kcs.KsCase(kc.case, kc.key_idx.copy(), kc.refused)
    R_ext = kcs.to_ext(kc.case.dirty["R"])
    t = where["good 8"]
    row = kc.case.row(t, 2)
    R_ext[row, 64:] = 0                                          # Z = 0: unusable, status 3 for that share
    rng = np.random.default_rng(1040)
    for i in range(0, kc.case.n, 5):                             # other rows: a Z that is not 1
        if i != row:
            zc = int(rng.integers(2, 1 << 62))
            u, v = (int.from_bytes(R_ext[i, 32 * k:32 * k + 32].tobytes(), "little") for k in (0, 1))
            if u < o.Q and v < o.Q:
                R_ext[i] = np.concatenate([mc._fe([u * zc % o.Q])[0], mc._fe([v * zc % o.Q])[0], mc._fe([zc])[0]])
    kc.R_ext = R_ext
    got = run_and_check(ks.handle, kc, "(d) extended", oracle=False, ext=True)
    # (the poisoned R enters the binding hash: the transcript's other shares fail, and its status is its first share's)
    assert got[0][row] == 3 and got[4][t] != 0 and not got[2][t].any()
    assert got[4][where["good 3"]] == 0 and got[4][where["index == n_keys"]] == 3


# ---- (e) ----
def _unaligned(a):
    a = np.ascontiguousarray(a)
    buf = np.empty(a.nbytes + 1, np.uint8)
    view = buf[1:].view(a.dtype).reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 2 == 1
    return view


@pytest.mark.parametrize("fmt", ["affine", "ext"])
def test_e_host_form_from_unaligned_views(ks, fmt):
    kc, where = call_a()
    idx, z, R, S, m, offs = kc.args()
    if fmt == "ext":
        R, S = kcs.to_ext(R), kcs.to_ext(S)
    ins = [_unaligned(x) for x in (idx, z, R, S, m, offs)]
    n, T = kc.case.n, kc.T
    outs = [_unaligned(np.full(s, FILL, np.uint8)) for s in ((n,), (T,), (T, 64), (T, 32), (T, 64))]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib().jjs_multisig_combine_keyset(ks.handle, 1 if fmt == "ext" else 0, *[p(x) for x in ins], T, *[p(x) for x in outs])
    assert rc == 0, lib().jjs_last_error()
    st, ts, agg, su, sr = outs
    got = (st, agg, su, sr, ts)
    written(got, "(e)")
    rc, want = keyset_call(ks.handle, kc, ext=fmt == "ext")
    assert rc == 0
    for name, x, y in zip(mc.OUTPUTS, got, want):
        assert (x == y).all(), (fmt, name)
    assert mc.check(kc.case, kcs.expected(kc, THREADS), got, "(e) " + fmt) == 0
    # the Python mirror's blocking route, and transcript_status = NULL
    mirror = ks.multisig_combine(idx, z, R, S, m, offs, fmt=fmt)
    for name, x, y in zip(mc.OUTPUTS, mirror, want):
        assert (np.asarray(x) == y).all(), (fmt, name, "mirror")
    outs2 = [_unaligned(np.full(s, FILL, np.uint8)) for s in ((n,), (T,), (T, 64), (T, 32), (T, 64))]
    rc = lib().jjs_multisig_combine_keyset(ks.handle, 1 if fmt == "ext" else 0, *[p(x) for x in ins], T, p(outs2[0]), None, *[p(x) for x in outs2[2:]])
    assert rc == 0 and (outs2[1] == FILL).all()
    for k in (0, 2, 3, 4):
        assert (outs2[k] == outs[k]).all()


# ---- (f) ----
def test_f_state_across_calls(eng, ks):
    import torch
    small, _ = call_a()
    big = call_8193()
    gc = gcs.group_transcripts(3, 20, seed=1050, threads=THREADS)
    gc.case.corrupt(4, 1)

    def others():
        a = gc.case.args()
        inl = tuple(t.cpu().numpy() for t in eng.multisig_combine(*[dev(x) for x in a[:5]], a[5]))
        with eng.multisig_group(gc.PK) as grp:
            g_out = tuple(t.cpu().numpy() for t in grp.combine(*[dev(x) for x in gc.call_args()]))
        return inl + g_out
    before = others()
    first = run_and_check(ks.handle, small, "(f) small", oracle=False)
    run_and_check(ks.handle, big, "(f) larger: the scratch grows", oracle=False)
    again = run_and_check(ks.handle, small, "(f) small again", oracle=False)
    for name, x, y in zip(mc.OUTPUTS, first, again):
        assert (x == y).all(), name
    after = others()
    for x, y in zip(before, after):
        assert (x == y).all(), "an existing call's bytes changed"
    mc.check(gc.case, mc.expected(gc.case, THREADS), before[:5], "(f) inline beside")
    # the torch route of the mirror
    idx, z, R, S, m, offs = small.args()
    mirror = ks.multisig_combine(dev(idx.view(np.int32)), dev(z), dev(R), dev(S), dev(m), offs)
    torch.cuda.synchronize()
    for name, x, y in zip(mc.OUTPUTS, mirror, first):
        assert (x.cpu().numpy() == y).all(), (name, "mirror")
    # a set registered from wire keys: the same bytes
    keys, _ = key_set()
    wire = np.stack([np.frombuffer(o.compress(to_pt(k)), np.uint8) for k in keys[:15]] + [np.full(32, 0xFF, np.uint8)])
    with eng.keyset("single", wire, fmt="wire") as ws:
        assert ws.key_status.tolist() == kcs.KEY_STATUS
        rc, got = keyset_call(ws.handle, small)
        assert rc == 0
        for name, x, y in zip(mc.OUTPUTS, got, first):
            assert (x == y).all(), (name, "wire-registered set")


# ---- (g) ----
def test_g_argument_errors(eng, ks):
    import torch
    kc = kcs.pool_transcripts([2, 1], 1060, *key_set(), threads=THREADS)
    keys, _ = key_set()
    idx, z, R, S, m, offs = kc.args()
    ins = [dev(idx.view(np.int32)), dev(z), dev(R), dev(S), dev(m)]
    outs = _outputs(kc.case.n, kc.T, FILL)
    st, ts, agg, su, sr = outs
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, fmt=0, T=kc.T, key_idx=ins[0]):
        return lib().jjs_multisig_combine_keyset_dev(h, fmt, _ptr(key_idx), *[_ptr(x) for x in ins[1:]], offs.ctypes.data_as(ctypes.c_void_p), T,
                                                     _ptr(st), _ptr(ts), _ptr(agg), _ptr(su), _ptr(sr), stream)

    def host_call(h, fmt=0, T=kc.T):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        o_ = [np.full(s, FILL, np.uint8) for s in ((kc.case.n,), (T,), (max(T, 1), 64), (max(T, 1), 32), (max(T, 1), 64))]
        rc = lib().jjs_multisig_combine_keyset(h, fmt, p(idx), p(z), p(R), p(S), p(m), p(offs), T, *[p(x) for x in o_])
        return rc, o_
    with eng.keyset("double", keys[:2], keys[2:4]) as dbl:
        assert call(dbl.handle) == -1 and host_call(dbl.handle)[0] == -1
        assert b"JJS_SCHEME_SINGLE" in lib().jjs_last_error()
    assert call(ks.handle, fmt=2) == -1 and host_call(ks.handle, fmt=2)[0] == -1
    gone = eng.keyset("single", keys[:3])
    stale = gone.handle
    gone.close()
    for h in (stale, 0, 12345):
        assert call(h) == -1 and host_call(h)[0] == -1, h
    assert call(ks.handle, key_idx=None) == -1
    assert call(ks.handle, T=0) == 0
    rc, o_ = host_call(ks.handle, T=0)
    assert rc == 0 and all((x == FILL).all() for x in o_)
    torch.cuda.synchronize()
    for x in outs:
        assert (x.cpu().numpy() == FILL).all(), "an argument error or an empty call wrote something"
    assert call(ks.handle) == 0
    got = host(outs)
    assert got[4].tolist() == [0, 0]


# ---- (h) ----
def test_h_second_trip_of_the_grid_stride_loop(ks):
    lanes = lib().jjs_debug_msig_resident_lanes()
    assert lanes > 0
    keys, sk = key_set()
    base = kcs.pool_transcripts([1] * 1024, 1070, keys, sk, threads=THREADS)
    base.case.corrupt(17, 0)
    base.refuse(33, 0, kcs.ORDER2_KEY, "order 2")
    reps = (lanes + 64) // 1024 + 1
    tiled = mc.tile(base.case, reps)
    n = lanes + 64
    kc = kcs.KsCase(tiled.slice(0, n), np.tile(base.key_idx, reps)[:n], {t + r * 1024: w for r in range(reps) for t, w in base.refused.items() if t + r * 1024 < n})
    assert kc.case.n == n == kc.T
    got = run_and_check(ks.handle, kc, f"(h) {n} shares, resident lanes {lanes}", oracle=False)
    st = got[0]
    assert (st.reshape(-1)[:(n // 1024) * 1024].reshape(-1, 1024) == st[:1024]).all() and st[17] == 4 and st[33] == 3 and st[n - 1] == st[(n - 1) % 1024]

"""Poseidon digests of ragged inputs on the MI355X (jjs_digest_dev, jjs_digest): the case lists of digest_cases.py through both
routes -- eight lanes per item and one -- on both sides of the boundary jjs_debug_digest_limits reports, uniform and ragged,
canonical and wide, truncated and not, against oracle poseidon_any bit for bit; the range test with its neighbours; the tie to
jjs_challenge_single_dev and to jjs_verify_single_dev; the host form; the arguments."""
import ctypes

import numpy as np
import pytest

import digest_cases as dc

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


@pytest.fixture(scope="module")
def limits(eng):
    lim = eng.digest_limits()
    assert 1 <= lim["coop_max_items"] < lim["grid_lanes"]
    return lim


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def offsets_ptr(case):
    if case["offsets"] is None:
        return None, None
    keep = np.ascontiguousarray(case["offsets"], np.uint32)
    return keep, keep.ctypes.data_as(P)


def dev_call(eng, case, flags=0, want_status=True):
    """jjs_digest_dev over outputs pre-filled with 0xA5 -> (out, status or None)"""
    import torch
    n = case["n"]
    inp = dev(case["in"])
    out = torch.full((max(n, 1), 32), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    keep, off = offsets_ptr(case)
    rc = eng._lib.jjs_digest_dev(case["fmt"], flags, P(inp.data_ptr()), off, case["k"], n, P(out.data_ptr()),
                                 P(status.data_ptr()) if want_status else None, eng._stream())
    assert rc == 0, eng._lib.jjs_last_error()
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    if not want_status:
        assert (st == 0xA5).all()
    return out.cpu().numpy()[:n], st[:n] if want_status else None


def host_call(eng, case, flags=0, want_status=True, skew=0):
    """jjs_digest from host buffers that start `skew` bytes off a 64-byte boundary"""
    n = case["n"]

    def buf(size):
        raw = np.full(size + 128, 0xA5, np.uint8)
        at = (-raw.ctypes.data) % 64 + skew
        return raw[at:at + size]
    inp = buf(case["in"].size)
    inp[...] = case["in"].reshape(-1)
    out, status = buf(32 * n), buf(n)
    assert skew == 0 or (inp.ctypes.data % 16 and out.ctypes.data % 16)
    keep, off = offsets_ptr(case)
    rc = eng._lib.jjs_digest(case["fmt"], flags, inp.ctypes.data_as(P), off, case["k"], n, out.ctypes.data_as(P),
                             status.ctypes.data_as(P) if want_status else None)
    assert rc == 0, eng._lib.jjs_last_error()
    return out.reshape(n, 32).copy(), status.copy() if want_status else None


def compare(got, case, flags, what):
    out, status = got
    want = dc.truncated(case["want"]) if flags & 1 else case["want"]
    rows = np.where((out != want).any(1))[0]
    assert len(rows) == 0, (what, rows[:8], case["status"][rows[:8]])
    if status is not None:
        bad = np.where(status != case["status"])[0]
        assert len(bad) == 0, (what, bad[:8], status[bad[:8]])


def both_routes(eng, limits, case, what, flags=(0, 1)):
    """the case as it is (the eight-lane route) and followed by filler items up to limit + 1 (the one-lane route)"""
    assert case["n"] <= limits["coop_max_items"]
    for c in (case, dc.padded(case, limits["coop_max_items"] + 1)):
        for f in flags:
            compare(dev_call(eng, c, f), c, f, (what, c["n"], f))


@pytest.mark.parametrize("k", dc.LENGTHS)
def test_uniform_lengths(eng, k):
    for n in dc.SIZES:
        case = dc.uniform(k, n)
        for flags in (0, 1):
            compare(dev_call(eng, case, flags), case, flags, (k, n, flags))
    assert (dev_call(eng, dc.uniform(k, 1))[0][0] == dc.python_digest(dc.uniform(k, 1)["values"], [0, k], 0)).all()


def test_every_length_on_both_routes(eng, limits):
    both_routes(eng, limits, dc.every_length(), "every length")


def test_uniform_long_tag_on_the_one_lane_route(eng, limits):
    """k = 1028 at limit + 1 items: one tag computed on the device for the whole call (long_stride 0), read by digest_kernel"""
    n = limits["coop_max_items"] + 1
    for k in (1027, 1028):
        case = dc.uniform_tiled(k, n)
        compare(dev_call(eng, case, 1), case, 1, ("uniform long", k, n))


def test_route_boundary_and_second_trip(eng, limits):
    limit, lanes = limits["coop_max_items"], limits["grid_lanes"]
    for n in (limit - 1, limit, limit + 1):
        case = dc.uniform(5, n)
        compare(dev_call(eng, case, 1), case, 1, ("boundary", n))
    case = dc.uniform(1, lanes + 1)                       # digest_kernel strides over its grid: one lane takes a second item
    compare(dev_call(eng, case), case, 0, ("second trip", lanes + 1))


@pytest.mark.parametrize("reverse", [False, True])
def test_ragged_on_both_routes(eng, limits, reverse):
    case = dc.ragged(reverse)
    both_routes(eng, limits, case, ("ragged", reverse))
    out, _ = dev_call(eng, case)
    at = case["n"] - 8 if reverse else 7
    assert (out[at] == dc.python_digest(case["values"], case["offs"], at)).all()


def test_equal_lengths_through_offsets_equal_the_uniform_call(eng, limits):
    for n in (65, limits["coop_max_items"] + 1):
        case = dc.uniform(5, n)
        a, sa = dev_call(eng, case)
        b, sb = dev_call(eng, dc.as_offsets(case))
        assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
        compare((a, sa), case, 0, n)


def test_range_test_on_both_routes(eng, limits):
    case = dc.range_test()
    assert (case["status"] == 3).sum() == 24 and (case["status"] == 0).sum() == case["n"] - 24
    both_routes(eng, limits, case, "range")
    for c in (case, dc.padded(case, limits["coop_max_items"] + 1)):
        compare(dev_call(eng, c, 0, want_status=False), c, 0, "status == NULL still zeroes the row")


def test_wide_on_both_routes(eng, limits):
    case = dc.wide()
    both_routes(eng, limits, case, "wide")
    out, status = dev_call(eng, dc.padded(case, limits["coop_max_items"] + 1))
    assert (status == 0).all()


def test_truncated_digest_is_the_single_challenge(eng):
    """jjs_digest_dev(..., TRUNCATED) over [R.u, R.v, PK.u, PK.v, m] == jjs_challenge_single_dev, which the reference's vectors pin"""
    import torch
    from helpers import make_batch
    b = make_batch("single", 65, seed=3, mix=False)
    rows = np.concatenate([b["R"], b["PK"], b["m"]], axis=1).reshape(65, 5, 32)
    got, status = eng.digest(dev(rows), truncated=True)
    want = eng.challenge("single", dev(b["R"]), dev(b["PK"]), dev(b["m"]))
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and (status.cpu().numpy() == 0).all()


def test_digests_are_the_m_column_of_verify(eng):
    """signatures the oracle made on the oracle's digests of random payloads verify against the device's digests"""
    import torch
    import jjs_oracle as o
    import jjs_oracle_c as oc
    from helpers import rand_mod
    rng = np.random.default_rng(12)
    n = 70
    lens = [1 + (11 * i) % 23 for i in range(n)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    payload = dc.rand_canonical(rng, int(offsets[-1]))
    m = dc.expected(payload, offsets.astype(np.int64))
    u, R, PK = oc.sign_single(rand_mod(rng, n, o.R_ORDER, nonzero=True), rand_mod(rng, n, o.R_ORDER), m)
    digests, st = eng.digest(dev(payload), lens)
    status, tally = eng.verify("single", dev(u), dev(R), dev(PK), digests)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (status.cpu().numpy() == 0).all() and tally.cpu().numpy().tolist() == [n, 0, 0, 0]
    assert digests.cpu().numpy().tobytes() == m.tobytes()


def test_host_form(eng, limits):
    """equals the device form, from unaligned buffers; a larger call grows the staging, the next ones reuse it"""
    small, big = dc.ragged(), dc.padded(dc.range_test(), limits["coop_max_items"] + 1)
    for case in (small, dc.wide(), dc.uniform(1028, 3)):
        for flags in (0, 1):
            for skew in (0, 1):
                got = host_call(eng, case, flags, skew=skew)
                compare(got, case, flags, ("host", case["n"], flags, skew))
                d = dev_call(eng, case, flags)
                assert got[0].tobytes() == d[0].tobytes() and got[1].tobytes() == d[1].tobytes()
    compare(host_call(eng, big, 0, skew=3), big, 0, "host, large")
    grown = eng.memory_stats()
    compare(host_call(eng, small, 0, want_status=False), small, 0, "host, no status")
    compare(host_call(eng, big, 1), big, 1, "host, large again")
    assert eng.memory_stats() == grown, "the second round allocates nothing"
    out, st = eng.digest(small["in"], np.diff(small["offs"]))
    assert out.tobytes() == small["want"].tobytes() and (st == 0).all()
    out, st = eng.digest(dc.uniform(5, 65)["in"].tobytes(), 5, truncated=True)
    assert out.tobytes() == dc.truncated(dc.uniform(5, 65)["want"]).tobytes()


def test_arguments(eng):
    import torch
    lib = eng._lib
    inp, out = dev(dc.uniform(5, 4)["in"]), torch.full((4, 32), 0xA5, dtype=torch.uint8, device="cuda")
    host_in, host_out = np.zeros((20, 32), np.uint8), np.full((4, 32), 0xA5, np.uint8)
    s = eng._stream()

    def offs(*v):
        return np.array(v, np.uint32)

    def both(fmt, flags, null_in, offsets, k, n, null_out=False):
        o_p = offsets.ctypes.data_as(P) if offsets is not None else None
        a = lib.jjs_digest_dev(fmt, flags, None if null_in else P(inp.data_ptr()), o_p, k, n, None if null_out else P(out.data_ptr()), None, s)
        b = lib.jjs_digest(fmt, flags, None if null_in else host_in.ctypes.data_as(P), o_p, k, n,
                           None if null_out else host_out.ctypes.data_as(P), None)
        assert a == b, (a, b)
        return a
    assert both(0, 0, False, None, 5, 4) == 0
    torch.cuda.synchronize()
    out.fill_(0xA5)
    host_out[...] = 0xA5
    for fmt in (2, -1, 7):
        assert both(fmt, 0, False, None, 5, 4) == -1
    for flags in (2, 3, 0x100, -2):
        assert both(0, flags, False, None, 5, 4) == -1
    assert both(0, 0, True, None, 5, 4) == -1 and both(0, 0, False, None, 5, 4, null_out=True) == -1
    assert both(0, 0, False, offs(1, 5, 10, 15, 20), 0, 4) == -1              # does not start at 0
    assert both(0, 0, False, offs(0, 5, 4, 15, 20), 0, 4) == -1               # decreases
    assert both(0, 0, False, offs(0, 5, 5, 15, 20), 0, 4) == -1               # an empty item
    assert both(0, 0, False, None, 0, 4) == -1                                # k = 0
    assert both(0, 0, False, None, 1 << 31, 4) == -1                          # beyond what the tag encodes
    assert both(0, 0, False, offs(0, 1 << 31, (1 << 31) + 1), 0, 2) == -1
    assert lib.jjs_digest_dev(0, 0, P(inp.data_ptr() + 8), None, 5, 3, P(out.data_ptr()), None, s) == -1      # misaligned
    assert lib.jjs_digest_dev(0, 0, P(inp.data_ptr()), None, 5, 3, P(out.data_ptr() + 4), None, s) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[3] == 0xA5).all() and (host_out[3] == 0xA5).all(), "a refused call writes nothing"
    out.fill_(0xA5)
    host_out[...] = 0xA5
    assert both(0, 0, False, None, 5, 0) == 0 and both(0, 0, True, None, 0, 0, null_out=True) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and (host_out == 0xA5).all(), "n == 0 writes nothing"
    lim = (ctypes.c_uint64 * 2)()
    assert lib.jjs_debug_digest_limits(lim) == 0 and lib.jjs_debug_digest_limits(None) == -1

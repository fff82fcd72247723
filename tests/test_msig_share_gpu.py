"""verify_share on its own on the device: the six entry points of include/jjs_gpu.h (inline, signer group, key set; device
columns and host buffers) through the C ABI with every output prefilled with 0xA5, in the three input formats, and the Python
mirrors.  Expected values are those of msig_share_cases: the C oracle's share_status with the query's z at its row, the oracles'
RSa, and the statuses 3 and 5 written out from the rules of the header -- never the code under test."""
import ctypes

import numpy as np
import pytest

import jjs_oracle as o
import jjs_oracle_c as oc
import msig_share_cases as shc
import multisig_cases as mc
from helpers import pt_bytes, to_int, to_pt

pytestmark = pytest.mark.gpu
THREADS = 16
FILL = 0xA5
H = bytes.fromhex


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


@pytest.fixture(scope="module")
def inline():
    sc = shc.inline_case()
    return sc, shc.expected_status(sc, THREADS), shc.expected_R(sc, THREADS)


@pytest.fixture(scope="module")
def groups(eng):
    out = []
    for name, sc in shc.group_cases():
        out.append((name, sc, shc.expected_status(sc, THREADS), shc.expected_R(sc, THREADS), eng.multisig_group(sc.group_pk)))
    yield out
    for entry in out:
        entry[4].close()


@pytest.fixture(scope="module")
def keyset(eng):
    sc = shc.keyset_case()
    ks = eng.keyset("single", sc.keys)
    yield sc, shc.expected_status(sc, THREADS), shc.expected_R(sc, THREADS), ks
    ks.close()


@pytest.fixture(scope="module")
def singles():
    """8 193 transcripts of one participant, one query each (every 11th share off by one); sig_R from the C oracle."""
    case = mc.valid_transcripts([1] * 8193, 77, threads=THREADS)
    sc = shc.ShareCase("inline", case)
    for t in range(case.T):
        z = to_int(case.clean["z"][t])
        sc.ask(t, 0, (z + 1) % o.R_ORDER if t % 11 == 3 else z)
    st, _, _, _, sr = oc.multisig_combine(*[case.clean[k] for k in mc.COLS], case.offsets.astype(np.uint32), threads=THREADS)
    assert not st.any()
    return sc, shc.expected_status(sc, THREADS), sr


def lib():
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def odd(a, dtype=np.uint8):
    """A copy at an odd address: the host forms ask for no alignment."""
    a = np.ascontiguousarray(a, dtype=dtype)
    raw = np.empty(a.nbytes + 8, np.uint8)
    out = raw[1:1 + a.nbytes].view(dtype).reshape(a.shape)
    out[...] = a
    return out


def head_and_columns(sc, fmt, handle):
    """The arguments in front of the queries: ints, numpy columns, and the offsets as ("host", array) -- host memory in both forms."""
    cols, m = sc.columns(fmt)
    offs = sc.case.offsets.astype(np.uint32)
    fid = shc.FORMAT_IDS[fmt]
    if sc.route == "inline":
        return "jjs_multisig_verify_share", [fid, cols["PK"], cols["R"], cols["S"], m, ("host", offs), sc.T]
    if sc.route == "group":
        return "jjs_msig_group_verify_share", [handle, fid, cols["R"], cols["S"], m, sc.T]
    return "jjs_multisig_verify_share_keyset", [handle, fid, sc.key_idx, cols["R"], cols["S"], m, ("host", offs), sc.T]


class DevCall:
    """One *_dev call: the inputs uploaded, the outputs prefilled.  launch() queues it on the current stream."""

    def __init__(self, sc, fmt="affine", handle=None, want_R=True):
        import torch
        self.sc = sc
        self.name, head = head_and_columns(sc, fmt, handle)
        self.keep = []
        self.args = []
        for a in head:
            if isinstance(a, np.ndarray):
                t = dev(a.view(np.int32) if a.dtype == np.uint32 else a)
                self.keep.append(t); self.args.append(_ptr(t))
            elif isinstance(a, tuple):
                self.keep.append(a[1]); self.args.append(_h(a[1]))
            else:
                self.args.append(a)
        qt, qs, z = sc.queries()
        self.q = [dev(qt.view(np.int32)), dev(qs.view(np.int32)), dev(z)]
        self.st = torch.full((max(sc.Q, 1),), FILL, dtype=torch.uint8, device="cuda")[:sc.Q]
        self.sr = torch.full((max(sc.T, 1), 64), FILL, dtype=torch.uint8, device="cuda")[:sc.T] if want_R else None

    def launch(self):
        import torch
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return getattr(lib(), self.name + "_dev")(*self.args, *[_ptr(x) for x in self.q], self.sc.Q, _ptr(self.st), _ptr(self.sr), stream)

    def read(self):
        import torch
        torch.cuda.synchronize()
        st, sr = self.st.cpu().numpy(), (self.sr.cpu().numpy() if self.sr is not None else None)
        assert not (st == FILL).any(), "a status was not written"
        assert sr is None or not (sr == FILL).all(1).any(), "a row of sig_R was not written"
        return st, sr


def run_dev(sc, fmt="affine", handle=None, want_R=True):
    call = DevCall(sc, fmt, handle, want_R)
    assert call.launch() == 0, lib().jjs_last_error()
    return call.read()


def run_host(sc, fmt="affine", handle=None, want_R=True):
    name, head = head_and_columns(sc, fmt, handle)
    keep = [odd(a, a.dtype) if isinstance(a, np.ndarray) else (a[1] if isinstance(a, tuple) else a) for a in head]
    qt, qs, z = (odd(a, a.dtype) for a in sc.queries())
    st = odd(np.full(sc.Q, FILL, np.uint8))
    sr = odd(np.full((sc.T, 64), FILL, np.uint8)) if want_R else None
    rc = getattr(lib(), name)(*[_h(a) if isinstance(a, np.ndarray) else a for a in keep], _h(qt), _h(qs), _h(z), sc.Q, _h(st), _h(sr))
    assert rc == 0, lib().jjs_last_error()
    assert not (st == FILL).any() and (sr is None or not (sr == FILL).all(1).any()), "an output row was not written"
    return st.copy(), (sr.copy() if sr is not None else None)


RUNS = {"dev": run_dev, "host": run_host}


@pytest.mark.parametrize("form", ("dev", "host"))
@pytest.mark.parametrize("fmt", shc.FORMATS)
def test_inline(eng, inline, fmt, form):
    sc, want, want_R = inline
    st, sr = RUNS[form](sc, fmt)
    shc.check(sc, want, want_R, st, sr, f"{fmt}, {form}")
    st2, none = RUNS[form](sc, fmt, want_R=False)
    assert none is None and (st2 == st).all()


@pytest.mark.parametrize("form", ("dev", "host"))
@pytest.mark.parametrize("fmt", shc.FORMATS)
def test_groups(eng, groups, fmt, form):
    for name, sc, want, want_R, grp in groups:
        calls = grp.info()["calls"]
        st, sr = RUNS[form](sc, fmt, grp.handle)
        shc.check(sc, want, want_R, st, sr, f"{name}, {fmt}, {form}")
        assert grp.info()["calls"] == calls + 1


@pytest.mark.parametrize("form", ("dev", "host"))
@pytest.mark.parametrize("fmt", shc.FORMATS)
def test_keyset(eng, keyset, fmt, form):
    sc, want, want_R, ks = keyset
    st, sr = RUNS[form](sc, fmt, ks.handle)
    shc.check(sc, want, want_R, st, sr, f"{fmt}, {form}")


def test_routes_agree(eng, inline, groups, keyset):
    """The same transcripts and queries: a group call against the inline call on the tiled keys, a key-set call against the inline
    call on the gathered keys (but for the refused transcripts)."""
    for name, sc, _, _, grp in groups:
        st, sr = run_dev(sc, "affine", grp.handle)
        ist, isr = run_dev(shc.as_route(sc, "inline"))
        assert (ist == st).all() and (isr == sr).all(), name
    sc, _, _, ks = keyset
    st, sr = run_dev(sc, "affine", ks.handle)
    ist, isr = run_dev(shc.as_route(sc, "inline"))
    ok_q = np.array([t >= sc.T or t not in sc.refused for t in sc.qt])
    ok_t = np.array([t not in sc.refused for t in range(sc.T)])
    assert (ist[ok_q] == st[ok_q]).all() and (isr[ok_t] == sr[ok_t]).all()
    assert (st[~ok_q] == 3).all() and not sr[~ok_t].any()


def test_agrees_with_combine(eng):
    """jjs_multisig_combine_dev's share_status row, with every query's z standing at its row: one query per row."""
    case = mc.valid_transcripts([3, 1, 5, 2], 31, threads=THREADS)
    case.corrupt(0, 2); case.corrupt(2, 0); case.corrupt(2, 4)
    sc = shc.ShareCase("inline", case)
    sc.ask_all()
    st, sr = run_dev(sc)
    cst, _, _, csr, cts = (x.cpu().numpy() for x in eng.multisig_combine(*[dev(x) for x in case.args()[:5]], case.args()[5]))
    assert (st == cst).all() and set(st.tolist()) == {0, 4}
    good = cts == 0
    assert good.tolist() == [False, True, False, True] and (sr[good] == csr[good]).all() and sr[~good].any(1).all()


def test_reference_kat(eng, reference_kat):
    kat = reference_kat["multisig_kat"]
    pts = lambda v: np.stack([pt_bytes(o.mul(o.G, x)) for x in v])  # noqa: E731
    PK, R, S = pts(kat["secret_keys"]), pts(kat["r_scalars"]), pts(kat["s_scalars"])
    assert [o.compress(to_pt(x)).hex() for x in PK] == kat["public_keys"]
    z = np.stack([np.frombuffer(H(x), np.uint8) for x in kat["individual_shares"]])
    case = mc.Case({"z": z, "PK": PK, "R": R, "S": S, "m": mc._fe([kat["message"]])}, [0, 3], [0, 0, 0])
    sc = shc.ShareCase("inline", case)
    sc.ask_all()
    sc.ask(0, 1, to_int(z[0]), "another signer's share")
    st, sr = run_dev(sc)
    assert st.tolist() == [0, 0, 0, 4]
    assert o.compress(to_pt(sr[0])).hex() == kat["aggregate_commitment"]
    # the mirrors: torch tensors and numpy arrays
    qt, qs, qz = sc.queries()
    got = eng.multisig_verify_share(dev(PK), dev(R), dev(S), dev(case.dirty["m"]), [0, 3], dev(qt.view(np.int32)), dev(qs.view(np.int32)), dev(qz),
                                    want_R=True)
    assert got[0].cpu().numpy().tolist() == [0, 0, 0, 4] and (got[1].cpu().numpy() == sr).all()
    assert eng.multisig_verify_share(PK, R, S, case.dirty["m"], [0, 3], qt, qs, qz).tolist() == [0, 0, 0, 4]
    with eng.multisig_group(PK) as grp:
        assert grp.verify_share(R, S, case.dirty["m"], qt, qs, qz).tolist() == [0, 0, 0, 4]
        got = grp.verify_share(dev(R), dev(S), dev(case.dirty["m"]), dev(qt.view(np.int32)), dev(qs.view(np.int32)), dev(qz), want_R=True)
        assert got[0].cpu().numpy().tolist() == [0, 0, 0, 4] and (got[1].cpu().numpy() == sr).all()
    with eng.keyset("single", PK) as ks:
        idx = np.arange(3, dtype=np.uint32)
        got = ks.multisig_verify_share(idx, R, S, case.dirty["m"], [0, 3], qt, qs, qz, want_R=True)
        assert got[0].tolist() == [0, 0, 0, 4] and (got[1] == sr).all()
        got = ks.multisig_verify_share(dev(idx.view(np.int32)), dev(R), dev(S), dev(case.dirty["m"]), [0, 3], dev(qt.view(np.int32)),
                                       dev(qs.view(np.int32)), dev(qz))
        assert got.cpu().numpy().tolist() == [0, 0, 0, 4]


def test_non_default_stream(eng, inline, groups, keyset):
    import torch
    s = torch.cuda.Stream()
    calls = [DevCall(inline[0]), DevCall(groups[0][1], "affine", groups[0][4].handle), DevCall(keyset[0], "affine", keyset[3].handle)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for c in calls:
            assert c.launch() == 0, lib().jjs_last_error()
    for c, (sc, want, want_R) in zip(calls, (inline[:3], groups[0][1:4], keyset[:3])):
        shc.check(sc, want, want_R, *c.read(), "non-default stream")


@pytest.mark.parametrize("Q", (255, 256, 257))
def test_one_block_of_queries(eng, Q):
    case = mc.valid_transcripts([2, 3, 1], 35, threads=THREADS)
    sc = shc.ShareCase("inline", case)
    rows = [(t, j) for t in range(3) for j in range(int(case.sizes()[t]))]
    for q in range(Q):
        t, j = rows[q % len(rows)]
        z = to_int(case.clean["z"][case.row(t, j)])
        sc.ask(t, j, (z + 1) % o.R_ORDER if q % 5 == 4 else z)
    want = shc.expected_status(sc, THREADS)
    assert want[-1] in (0, 4) and {0, 4} == set(want.tolist())
    st, sr = run_dev(sc)
    shc.check(sc, want, shc.expected_R(sc), st, sr, f"Q = {Q}")


def _head(sc, T):
    """The first T transcripts of a case with one query per transcript of one participant."""
    x = shc.ShareCase("inline", sc.case.slice(0, T))
    x.qt, x.qs, x.qz, x.what = sc.qt[:T], sc.qs[:T], sc.qz[:T], sc.what[:T]
    return x


def test_hash_lane_modes_and_regrowth(eng, singles, inline):
    """B = 8 192 (eight lanes per transcript in the sums pass) and 8 193 (one); the larger call is queued straight behind a small
    one on the same stream and enlarges the scratch the small one still uses: both results are read afterwards."""
    sc, want, want_R = singles
    x = _head(sc, 8192)
    st, sr = run_dev(x)
    shc.check(x, want[:8192], want_R[:8192], st, sr, "B = 8192")
    small, big = DevCall(inline[0]), DevCall(sc)
    assert small.launch() == 0 and big.launch() == 0, lib().jjs_last_error()
    shc.check(inline[0], inline[1], inline[2], *small.read(), "the small call in front")
    shc.check(sc, want, want_R, *big.read(), "B = 8193")


def test_generated_and_computed_tags(eng):
    """One transcript of 256 participants (the last row of the generated SAFE tag table) and one of 257 (tags computed on the
    device) with three queries; sig_R from the C oracle on the valid transcripts."""
    case = mc.valid_transcripts([256, 257], 36, threads=THREADS)
    sc = shc.ShareCase("inline", case)
    sc.ask(1, 256)
    sc.ask(0, 128, (to_int(case.clean["z"][case.row(0, 128)]) + 1) % o.R_ORDER, "corrupted")
    sc.ask(0, 255)
    want = shc.expected_status(sc, THREADS)
    assert want.tolist() == [0, 4, 0]
    st, sr = run_dev(sc)
    shc.check(sc, want, shc.expected_R(sc, THREADS), st, sr)


def test_more_queries_than_rows_and_none(eng):
    case = mc.valid_transcripts([1, 2], 37, threads=THREADS)
    sc = shc.ShareCase("inline", case)
    for q in range(40):
        t, j = ((0, 0), (1, 0), (1, 1))[q % 3]
        z = to_int(case.clean["z"][case.row(t, j)])
        sc.ask(t, j, (z + q % 2) % o.R_ORDER)
    want, want_R = shc.expected_status(sc, THREADS), shc.expected_R(sc)
    for form in ("dev", "host"):
        shc.check(sc, want, want_R, *RUNS[form](sc), form)
    # no queries: sig_R is still filled; without sig_R nothing is written and nothing is wrong
    none = shc.ShareCase("inline", case)
    for form in ("dev", "host"):
        st, sr = RUNS[form](none)
        assert st.shape == (0,) and (sr == want_R).all(), form
        st, sr = RUNS[form](none, want_R=False)
        assert st.shape == (0,) and sr is None

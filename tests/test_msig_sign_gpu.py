"""jjs_multisig_round1_dev, jjs_multisig_sign_dev and jjs_multisig_sign on the device, through the C ABI with every output
prefilled with 0xA5.  Expected values: the reference's KAT bytes, the Python model of msig_sign_cases (sign_round_2 written out
over oracle/jjs_oracle.py) and, for whole calls, jjs_multisig_combine_dev, which must accept every generated share."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import jjs_oracle as o
import msig_sign_cases as sc
import multisig_cases as mc
from helpers import to_pt

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


def lib():
    from jubjub_schnorr_amd import _ffi
    return _ffi.lib()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _h(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class SignCall:
    """One jjs_multisig_sign_dev call: the inputs uploaded, the outputs prefilled.  launch() queues it on the current stream,
    read() gives numpy copies after a synchronisation."""

    def __init__(self, c, signer_row, sk, r, s):
        import torch
        self.c, self.k = c, len(sk)
        self.cols = [dev(x) for x in (c.PK, c.R, c.S, c.m)]
        self.rows = dev(signer_row.view(np.int32)) if signer_row is not None else None
        self.secrets = [dev(x) for x in (sk, r, s)]
        self.z = torch.full((max(self.k, 1), 32), FILL, dtype=torch.uint8, device="cuda")[:self.k]
        self.st = torch.full((max(self.k, 1),), FILL, dtype=torch.uint8, device="cuda")[:self.k]
        self.offs = c.offs32()

    def launch(self, fmt=None, B=None, k=None):
        fmt = int(self.c.fmt == "ext") if fmt is None else fmt
        return lib().jjs_multisig_sign_dev(fmt, *[_ptr(x) for x in self.cols], _h(self.offs), self.c.B if B is None else B, _ptr(self.rows),
                                           *[_ptr(x) for x in self.secrets], self.k if k is None else k, _ptr(self.z), _ptr(self.st), _stream())

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.z.cpu().numpy(), self.st.cpu().numpy()


def sign_dev(c, signer_row, sk, r, s):
    call = SignCall(c, signer_row, sk, r, s)
    assert call.launch() == 0, lib().jjs_last_error()
    z, st = call.read()
    assert not (z == FILL).all(1).any() and not (st == FILL).any(), "an output row was not written"
    return z, st


def sign_host(c, signer_row, sk, r, s):
    """jjs_multisig_sign from pageable buffers at odd addresses: the host form asks for no alignment."""
    def odd(a, dtype=np.uint8):
        a = np.ascontiguousarray(a, dtype=dtype)
        raw = np.empty(a.nbytes + 8, np.uint8)
        out = raw[1:1 + a.nbytes].view(dtype).reshape(a.shape)
        out[...] = a
        return out
    cols = [odd(x) for x in (c.PK, c.R, c.S, c.m)]
    secrets = [odd(x) for x in (sk, r, s)]
    rows = odd(signer_row, np.uint32) if signer_row is not None else None
    k = len(sk)
    z, st = odd(np.full((k, 32), FILL, np.uint8)), odd(np.full(k, FILL, np.uint8))
    offs = c.offs32()
    rc = lib().jjs_multisig_sign(int(c.fmt == "ext"), *[_h(x) for x in cols], _h(offs), c.B, _h(rows), *[_h(x) for x in secrets], k, _h(z), _h(st))
    assert rc == 0, lib().jjs_last_error()
    assert not (z == FILL).all(1).any() and not (st == FILL).any(), "an output row was not written"
    return z.copy(), st.copy()


def combine_dev(eng, c, z):
    """jjs_multisig_combine[_ext]_dev on the case's transcripts and these shares: numpy (share_status, agg_pk, sig_u, sig_R, transcript_status)."""
    import torch
    out = eng.multisig_combine(*[dev(x) for x in sc.combine_args(c, z)[:5]], c.offs32(), fmt=c.fmt)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")) as f:
        return json.load(f)["multisig_kat"]


@functools.lru_cache(None)
def ragged_with_model(fmt):
    c = sc.ragged(threads=THREADS)
    x = c.to_ext(77) if fmt == "ext" else c
    rows = [13, 0, 4, 2, 2]
    return x, sc.model(x, *x.call()), rows, sc.model(x, *x.call(rows))


@functools.lru_cache(None)
def rules():
    base, cases = sc.rule_cases(threads=THREADS)
    base_z, base_st = sc.model(base, *base.call(list(range(base.n))))
    assert not base_st.any()
    return base_z, cases, [sc.model(x.case, x.signer_row, x.sk, x.r, x.s) for x in cases]


@pytest.mark.parametrize("form", ("dev", "host"))
def test_reference_kat(eng, kat, form):
    c = sc.kat_case(kat)
    want = np.stack([np.frombuffer(H(x), np.uint8) for x in kat["individual_shares"]])
    sign = sign_dev if form == "dev" else sign_host
    z, st = sign(c, *c.call())
    assert st.tolist() == [0, 0, 0] and (z == want).all(), "signer_row NULL"
    z, st = sign(c, *c.call([2, 0]))
    assert st.tolist() == [0, 0] and (z == want[[2, 0]]).all(), "signer_row [2, 0]"
    x = c.to_ext(5)
    z, st = sign(x, *x.call())
    assert st.tolist() == [0, 0, 0] and (z == want).all(), "extended"


@pytest.mark.parametrize("form", ("dev", "host"))
@pytest.mark.parametrize("fmt", ("affine", "ext"))
def test_ragged_call(eng, fmt, form):
    x, want_all, rows, want_rows = ragged_with_model(fmt)
    sign = sign_dev if form == "dev" else sign_host
    z, st = sign(x, *x.call())
    sc.check((z, st), want_all, f"{fmt} {form}, signer_row NULL")
    assert not st.any()
    sc.check(sign(x, *x.call(rows)), want_rows, f"{fmt} {form}, signer_row given")
    share_st, _, su, _, ts = combine_dev(eng, x, z)
    assert not share_st.any() and ts.tolist() == [0, 0, 5, 0, 0]
    for t in (0, 1, 3, 4):
        assert (su[t] == sc.sum_mod_r(z[x.rows_of(t)])).all(), t


def test_every_rule(eng):
    base_z, cases, wants = rules()
    assert len(cases) == 17
    for rule, want in zip(cases, wants):
        got = sign_dev(rule.case, rule.signer_row, rule.sk, rule.r, rule.s)
        sc.check_rule(rule, base_z, got, "dev")
        sc.check(got, want, rule.name)
    rule = cases[-1]                                    # and one of them from host buffers: a duplicate together with a bad encoding
    sc.check(sign_host(rule.case, rule.signer_row, rule.sk, rule.r, rule.s), wants[-1], "host " + rule.name)


def test_duplicates_across_transcripts(eng):
    c = sc.across_transcripts(threads=THREADS)
    got = sign_dev(c, *c.call())
    assert not got[1].any() and got[0].any(1).all()
    sc.check(got, sc.model(c, *c.call()))


def test_arguments(eng):
    c = sc.ragged(threads=THREADS)
    call = SignCall(c, *c.call())
    assert call.launch(fmt=2) == -1, "JJS_FORMAT_WIRE"
    assert call.launch(k=c.n - 1) == -1, "signer_row NULL with n_signing != N"
    assert call.launch(B=0) == 0 and call.launch(k=0) == 0
    z, st = call.read()
    assert (z == FILL).all() and (st == FILL).all(), "a refused or empty call wrote something"


def test_one_lane_per_hash(eng):
    """4 200 transcripts of 2 participants: 8 400 rows, above MSIG_COOP_MAX_ITEMS, so pass 1 takes one lane per hash (the calls
    above run eight)."""
    c = sc.build([2] * 4200, 1700, THREADS)
    assert mc.lane_modes(c.n, c.B) == (1, 8, 8)
    z, st = sign_dev(c, *c.call())
    assert not st.any()
    sample = np.linspace(0, c.B - 1, 64).astype(int)
    rows = [i for t in sample for i in c.rows_of(t)]
    wz, wst = sc.model(c, *c.call(rows))
    sc.check((z[rows], st[rows]), (wz, wst), "a sample of 64 transcripts")
    share_st, _, _, _, ts = combine_dev(eng, c, z)
    assert not share_st.any() and not ts.any()


def test_257_participants(eng):
    """One past the generated tag table: clean against the model's recorded shares (msig_sign_cases.recorded_257, which the CPU
    build is checked against too), and S duplicated at rows 0 and 256, the two ends of the scan."""
    c = sc.long_case(THREADS)
    z, st = sign_dev(c, *c.call())
    sc.check((z, st), sc.model(c, *c.call(), recorded=sc.recorded_257(c)), "257")
    assert not st.any()
    d = c.copy()
    d.S[256] = d.S[0]; d.s[256] = d.s[0]
    z, st = sign_dev(d, *d.call())
    assert st.tolist() == [7] * 257 and not z.any()


def test_1000_participants(eng):
    """Checked by jjs_multisig_combine_dev alone (the Python model would take minutes): every share accepted, and sig_u the sum of
    the shares mod r, computed here."""
    c = sc.build([1000], 1800, THREADS)
    z, st = sign_dev(c, *c.call())
    assert not st.any()
    share_st, _, su, _, ts = combine_dev(eng, c, z)
    assert not share_st.any() and ts.tolist() == [0] and (su[0] == sc.sum_mod_r(z)).all()


def test_round1(eng):
    import torch
    rng = np.random.default_rng(1900)
    ks = [0, 1, o.R_ORDER - 1] + mc._scalars(rng, 61)
    r, s = mc._fe(ks), mc._fe(ks[::-1])
    r[40] = mc._fe([o.R_ORDER])[0]
    s[50] = mc._fe([mc.ALL_ONES])[0]
    R = torch.full((64, 64), FILL, dtype=torch.uint8, device="cuda")
    S, bad = R.clone(), torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    dr, ds = dev(r), dev(s)
    assert lib().jjs_multisig_round1_dev(_ptr(dr), _ptr(ds), 64, _ptr(R), _ptr(S), _ptr(bad), _stream()) == 0, lib().jjs_last_error()
    torch.cuda.synchronize()
    R, S, bad = R.cpu().numpy(), S.cpu().numpy(), bad.cpu().numpy()
    assert bad.tolist() == [int(i in (40, 50)) for i in range(64)]
    for i in range(64):
        if bad[i]:
            assert not R[i].any() and not S[i].any(), i
        else:
            assert to_pt(R[i]) == o.mul(o.G, ks[i]) and to_pt(S[i]) == o.mul(o.G, ks[63 - i]), i
    R2, S2, bad2 = eng.multisig_sign_round1(dr, ds)
    torch.cuda.synchronize()
    assert (R2.cpu().numpy() == R).all() and (S2.cpu().numpy() == S).all() and (bad2.cpu().numpy() == bad).all()
    assert lib().jjs_multisig_round1_dev(_ptr(dr), _ptr(ds), 64, _ptr(R2), _ptr(S2), None, _stream()) == 0, "bad_out is nullable"
    torch.cuda.synchronize()


def test_state_across_calls(eng):
    """A signing call, a combine call and a signing call again on one stream, all through slot 0's scratch, without a
    synchronisation between them: the flags of the first call (a duplicate, a repeated key, a bad encoding) do not reach the third."""
    import torch
    base_z, cases, wants = rules()
    by_name = {x.name: (x, w) for x, w in zip(cases, wants)}
    x, want_x = ragged_with_model("affine")[:2]
    dirty = [by_name[k] for k in ("a duplicate together with a bad encoding", "the signer's key at another row as well",
                                  "R duplicated between two participants")]
    first = [SignCall(r.case, r.signer_row, r.sk, r.r, r.s) for r, _ in dirty]
    clean = SignCall(x, *x.call())
    good_z = dev(want_x[0])
    for call in first:
        assert call.launch() == 0
    comb = eng.multisig_combine(good_z, *clean.cols, x.offs32())
    assert clean.launch() == 0
    comb2 = eng.multisig_combine(good_z, *clean.cols, x.offs32())
    torch.cuda.synchronize()
    for call, (r, want) in zip(first, dirty):
        sc.check(call.read(), want, r.name)
    sc.check(clean.read(), want_x, "the clean call behind them")
    for out in (comb, comb2):
        assert not out[0].cpu().numpy().any() and out[4].cpu().numpy().tolist() == [0, 0, 5, 0, 0]
    assert all((a.cpu().numpy() == b.cpu().numpy()).all() for a, b in zip(comb, comb2))


def test_python_mirror(eng):
    import torch
    x, want_all, rows, want_rows = ragged_with_model("ext")
    z, st = eng.multisig_sign_round2(x.PK, x.R, x.S, x.m, x.offs32(), x.sk, x.r, x.s, fmt="ext")
    sc.check((z, st), want_all, "numpy")
    rr, sk, r, s = x.call(rows)
    z, st = eng.multisig_sign_round2(*[dev(a) for a in (x.PK, x.R, x.S, x.m)], x.offs32(), dev(sk), dev(r), dev(s),
                                     signer_row=dev(rr.view(np.int32)), fmt="ext")
    torch.cuda.synchronize()
    sc.check((z.cpu().numpy(), st.cpu().numpy()), want_rows, "torch")

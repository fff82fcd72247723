"""jjs_multisig_aggregate_pk* and jjs_multisig_verify* on the device.  Every call is compared with the fixed definitions of
include/jjs_gpu.h for its refused and empty vectors and, in the same process, with jjs_multisig_combine_dev's agg_pk (canonical
dummy shares: z = 0, m = 0, R = S = the identity) and jjs_verify_single_dev's statuses on the same columns; the small calls
with jjs_oracle_c as well (msig_verify_cases.expected).  The key set is the 16 keys of msig_keyset_cases.key_set."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import jjs_oracle as o
import msig_group_cases as gcs
import msig_keyset_cases as kcs
import msig_verify_cases as vc
import multisig_cases as mc
from helpers import pt_bytes

pytestmark = pytest.mark.gpu
THREADS = 16
FILL = 0xA5
FORMS = ("inline", "keyset")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Call:
    """One call on the device: the inputs uploaded, the outputs prefilled.  launch() queues it on the current stream; read()
    gives numpy copies (after a synchronisation).  ext: the ExtV whose columns replace PK and R."""

    def __init__(self, form, c, handle=0, ext=None, verify=True, status=True, tally=True):
        import torch
        self.form, self.c, self.handle, self.ext, self.verify = form, c, handle, ext is not None, verify
        PK, R = (ext.PK, ext.R) if ext is not None else (c.PK, c.R)
        self.keys = dev(c.key_idx.view(np.int32)) if form == "keyset" else dev(PK)
        self.sig = [dev(c.u), dev(R), dev(c.m)] if verify else []
        full = lambda *shape: torch.full(shape, FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
        B = c.B
        self.agg, self.vst, self.st = full(max(B, 1), 64)[:B], full(max(B, 1))[:B], full(max(B, 1))[:B]
        self.tally = torch.full((4,), -6, dtype=torch.int64, device="cuda")
        self.want_status, self.want_tally = status, tally
        self.offs = c.offs32()

    def launch(self, B=None, fmt=None, keys="own", agg="own", handle=None):
        B = self.c.B if B is None else B
        fmt = (1 if self.ext else 0) if fmt is None else fmt
        keys = self.keys if isinstance(keys, str) else keys
        agg = self.agg if isinstance(agg, str) else agg
        ap = agg if isinstance(agg, ctypes.c_void_p) else _ptr(agg)
        h = self.handle if handle is None else handle
        po = self.offs.ctypes.data_as(ctypes.c_void_p)
        kp = keys if isinstance(keys, ctypes.c_void_p) else _ptr(keys)
        if not self.verify:
            if self.form == "keyset":
                return lib().jjs_multisig_aggregate_pk_keyset_dev(h, kp, po, B, ap, _ptr(self.vst), _stream())
            return lib().jjs_multisig_aggregate_pk_dev(fmt, kp, po, B, ap, _ptr(self.vst), _stream())
        tail = [B, ap, _ptr(self.st) if self.want_status else None, _ptr(self.tally) if self.want_tally else None, _stream()]
        if self.form == "keyset":
            return lib().jjs_multisig_verify_keyset_dev(h, fmt, kp, po, *[_ptr(x) for x in self.sig], *tail)
        return lib().jjs_multisig_verify_dev(fmt, kp, po, *[_ptr(x) for x in self.sig], *tail)

    def read(self):
        import torch
        torch.cuda.synchronize()
        out = {"agg": self.agg.cpu().numpy(), "vst": self.vst.cpu().numpy(), "st": self.st.cpu().numpy(),
               "tally": self.tally.cpu().numpy().astype(np.uint64)}
        return out

    def untouched(self):
        out = self.read()
        return all((out[k] == FILL).all() for k in ("agg", "vst", "st")) and (self.tally.cpu().numpy() == -6).all()


def reference_route(c, derived_R=None):
    """What the calls a verifier had before give on the same columns: jjs_multisig_combine_dev's agg_pk on the keys with dummy shares
    (the identity for an empty vector, which combine rejects), then jjs_verify_single_dev on it; the refused vectors by the
    fixed definition."""
    import torch
    B, n = c.B, c.n
    agg = np.tile(vc.IDENT, (B, 1))
    if n:
        ident = dev(np.tile(vc.IDENT, (n, 1)))
        zero = lambda rows, w: torch.zeros((max(rows, 1), w), dtype=torch.uint8, device="cuda")[:rows]  # noqa: E731
        z0, m0, pk = zero(n, 32), zero(B, 32), dev(c.PK_clean)         # (named: the tensors live until the call has run)
        st_, ts_ = zero(n, 1).reshape(-1), zero(B, 1).reshape(-1)
        a_, su_, sr_ = zero(B, 64), zero(B, 32), zero(B, 64)
        rc = lib().jjs_multisig_combine_dev(_ptr(z0), _ptr(pk), _ptr(ident), _ptr(ident), _ptr(m0), c.offs32().ctypes.data_as(ctypes.c_void_p), B,
                                            _ptr(st_), _ptr(ts_), _ptr(a_), _ptr(su_), _ptr(sr_), _stream())
        assert rc == 0, lib().jjs_last_error()
        torch.cuda.synchronize()
        full = c.sizes() > 0
        agg[full] = a_.cpu().numpy()[full]
    st_d = torch.zeros(max(B, 1), dtype=torch.uint8, device="cuda")[:B]
    tally = torch.zeros(4, dtype=torch.int64, device="cuda")
    cols = [dev(x) for x in (c.u, c.R if derived_R is None else derived_R, agg, c.m)]
    rc = lib().jjs_verify_single_dev(*[_ptr(x) for x in cols], B, _ptr(st_d), _ptr(tally), _stream())
    assert rc == 0, lib().jjs_last_error()
    torch.cuda.synchronize()
    st = st_d.cpu().numpy().copy()
    ok = c.usable()
    agg[~ok] = 0
    st[~ok] = 3
    return agg, np.where(ok, 0, 3).astype(np.uint8), st, np.bincount(st, minlength=4).astype(np.uint64)


def compare(got, want, label, verify=True):
    agg, vst, st, tally = want
    bad = np.nonzero((got["agg"] != agg).any(1))[0]
    assert not len(bad), (label, "agg_pk", bad[:8].tolist())
    if verify:
        bad = np.nonzero(got["st"] != st)[0]
        assert not len(bad), (label, "status", bad[:8].tolist(), got["st"][bad[:8]].tolist(), st[bad[:8]].tolist())
        assert got["tally"].tolist() == tally.tolist(), (label, "tally")
    else:
        assert (got["vst"] == vst).all(), (label, "vec_status")


def run_and_check(form, c, handle, label, oracle=True, ext=None):
    """Both operations of one case, against the reference route and (oracle) jjs_oracle_c; returns the verification's outputs."""
    derived = ext.derived_R if ext is not None else None
    ref = reference_route(c, derived)
    want = vc.expected(c, THREADS, derived) if oracle else None
    out = None
    for verify in (False, True):
        if ext is not None and form == "keyset" and not verify:
            continue                       # the key-set aggregation takes no point column: it has no extended format
        call = Call(form, c, handle, ext=ext, verify=verify)
        assert call.launch() == 0, (label, lib().jjs_last_error())
        out = call.read()
        assert not (out["agg"] == FILL).all(1).any(), (label, "an agg_pk row was not written")
        assert not (out["st" if verify else "vst"] == FILL).any(), (label, "a status was not written")
        compare(out, ref, label + " / reference route", verify)
        if oracle:
            compare(out, want, label + " / oracle", verify)
    print(f"{label}: rows={c.n} B={c.B} refused={len(c.refused)} tally={out['tally'].tolist()}")
    return out


@functools.lru_cache(None)
def mix(form):
    keys, sk = key_set()
    return vc.standard_mix(keys, sk, form, threads=THREADS)


def handle_of(form, ks):
    return ks.handle if form == "keyset" else 0


# ---- (a) ----
@pytest.mark.parametrize("form", FORMS)
def test_a_standard_mix(ks, form):
    c = mix(form)
    out = run_and_check(form, c, handle_of(form, ks), f"(a) {form}")
    vc.check_named(c, form, out["agg"], out["st"], form)
    for status, tally in ((False, True), (True, False)):
        call = Call(form, c, handle_of(form, ks), status=status, tally=tally)
        assert call.launch() == 0
        again = call.read()
        assert (again["agg"] == out["agg"]).all()
        if status:
            assert (again["st"] == out["st"]).all() and (call.tally.cpu().numpy() == -6).all(), "tally = NULL, and the buffer was written"
        else:
            assert again["tally"].tolist() == out["tally"].tolist() and (again["st"] == FILL).all(), "status = NULL, and the buffer was written"


# ---- (b) ----
@functools.lru_cache(None)
def ragged_8193(form):
    keys, sk = key_set()
    return vc.ragged(mc.COOP_MAX_ITEMS + 1, 1210, keys, sk, form, threads=THREADS, refusals=4)


@pytest.mark.parametrize("form", FORMS)
def test_b_both_hash_lane_modes_of_pass_1(ks, form):
    one = ragged_8193(form)
    assert one.n == mc.COOP_MAX_ITEMS + 1 and len(one.refused) == 4
    run_and_check(form, one, handle_of(form, ks), f"(b) {form} 8193 rows: one lane per row", oracle=False)
    keys, sk = key_set()
    eight = vc.ragged(mc.COOP_MAX_ITEMS, 1212, keys, sk, form, threads=THREADS, refusals=4)
    assert eight.n == mc.COOP_MAX_ITEMS
    run_and_check(form, eight, handle_of(form, ks), f"(b) {form} 8192 rows: eight lanes per row", oracle=False)


# ---- (c) ----
@pytest.mark.parametrize("form", FORMS)
def test_c_257_keys_in_one_vector(ks, form):
    keys, sk = key_set()
    rng = np.random.default_rng(1220)
    picks = [vc.draw(rng, n) for n in (3, mc.TABLE_PARTICIPANTS + 1, 2, 1, 2)]     # 257 > 12: drawn with repetition
    c = vc.build(picks, 1221, keys, sk, THREADS)
    c.spoil_u(3)
    if form == "inline":
        c.refuse_inline(2, 1, "off the curve")
    else:
        c.refuse_keyset(2, 1, 0xFFFFFFFF, "index 0xFFFFFFFF")
    out = run_and_check(form, c, handle_of(form, ks), f"(c) {form} long tags")
    assert out["st"].tolist() == [0, 0, 3, 2, 0]


# ---- (d) ----
@functools.lru_cache(None)
def one_key_base(form):
    keys, sk = key_set()
    rng = np.random.default_rng(1230)
    base = vc.build([vc.draw(rng, 1) for _ in range(1024)], 1231, keys, sk, THREADS)
    base.spoil_u(17)
    if form == "inline":
        base.refuse_inline(33, 0, "u coordinate >= q")
    else:
        base.refuse_keyset(33, 0, kcs.ORDER2_KEY, "order 2")
    return base


def one_key_vectors(form, B):
    base = one_key_base(form)
    t = vc.tile(base, (B + 1023) // 1024)
    refused = {k: w for k, w in t.refused.items() if k < B}
    return vc.VCase(t.PK[:B], t.key_idx[:B], t.offsets[:B + 1], t.u[:B], t.R[:B], t.m[:B], t.PK_clean[:B], refused)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [16384, 16385])
def test_d_verification_stage_on_either_side_of_its_boundary(ks, form, B):
    c = one_key_vectors(form, B)
    assert c.B == B == c.n
    out = run_and_check(form, c, handle_of(form, ks), f"(d) {form} B={B}", oracle=False)
    st = out["st"]
    assert st[17] == 2 and st[33] == 3 and st[0] == 0 and (st[:16384].reshape(-1, 1024) == st[:1024]).all() and st[B - 1] == st[(B - 1) % 1024]
    assert vc.expected(one_key_base(form), THREADS)[2].tolist() == st[:1024].tolist()


# ---- (e) ----
@pytest.mark.parametrize("form", FORMS)
def test_e_extended_format(ks, form):
    keys, sk = key_set()
    x = vc.ext_mix(keys, sk, form, threads=THREADS)
    c = x.case
    out = run_and_check(form, c, handle_of(form, ks), f"(e) {form} extended", ext=x)
    vc.check_named(c, form, out["agg"], out["st"], form + " ext")
    assert out["st"][c.where["R Z=0"]] == 3 and out["agg"][c.where["R Z=0"]].any()
    if form == "inline":
        assert out["st"][c.where["key Z=0"]] == 3 and not out["agg"][c.where["key Z=0"]].any()


# ---- (f) ----
def _unaligned(a):
    a = np.ascontiguousarray(a)
    buf = np.empty(a.nbytes + 1, np.uint8)
    view = buf[1:].view(a.dtype).reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 2 == 1
    return view


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt", ["affine", "ext"])
def test_f_host_forms_from_unaligned_views(eng, ks, form, fmt):
    keys, sk = key_set()
    x = vc.ext_mix(keys, sk, form, threads=THREADS) if fmt == "ext" else None
    c = x.case if x else mix(form)
    want = vc.expected(c, THREADS, x.derived_R if x else None)
    PK, R = (x.PK, x.R) if x else (c.PK, c.R)
    rows = c.key_idx if form == "keyset" else PK
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    ins = [_unaligned(a) for a in (rows, c.offs32(), c.u, R, c.m)]
    B, f = c.B, 1 if fmt == "ext" else 0
    agg, st, vst = (_unaligned(np.full(s, FILL, np.uint8)) for s in ((B, 64), (B,), (B,)))
    tally = _unaligned(np.full(4, 7, np.uint64))
    if form == "keyset":
        rc = lib().jjs_multisig_verify_keyset(ks.handle, f, *[p(a) for a in ins], B, p(agg), p(st), p(tally))
    else:
        rc = lib().jjs_multisig_verify(f, *[p(a) for a in ins], B, p(agg), p(st), p(tally))
    assert rc == 0, lib().jjs_last_error()
    compare({"agg": agg, "st": st, "tally": tally}, want, f"(f) {form} {fmt} verify")
    if not (form == "keyset" and fmt == "ext"):
        agg2 = _unaligned(np.full((B, 64), FILL, np.uint8))
        if form == "keyset":
            rc = lib().jjs_multisig_aggregate_pk_keyset(ks.handle, p(ins[0]), p(ins[1]), B, p(agg2), p(vst))
        else:
            rc = lib().jjs_multisig_aggregate_pk(f, p(ins[0]), p(ins[1]), B, p(agg2), p(vst))
        assert rc == 0, lib().jjs_last_error()
        compare({"agg": agg2, "vst": vst}, want, f"(f) {form} {fmt} aggregate", verify=False)
    # status and tally NULL: the aggregates alone
    agg3 = np.full((B, 64), FILL, np.uint8)
    if form == "keyset":
        rc = lib().jjs_multisig_verify_keyset(ks.handle, f, *[p(a) for a in ins], B, p(agg3), None, None)
    else:
        rc = lib().jjs_multisig_verify(f, *[p(a) for a in ins], B, p(agg3), None, None)
    assert rc == 0 and (agg3 == want[0]).all()
    # both mirrors' blocking routes
    owner = ks if form == "keyset" else eng
    mst, mtally, magg = owner.multisig_verify(rows, c.offs32(), c.u, R, c.m, fmt=fmt)
    compare({"agg": magg, "st": mst, "tally": mtally}, want, f"(f) {form} {fmt} mirror verify")
    if form == "inline":
        magg, mvst = eng.multisig_aggregate_pk(rows, c.offs32(), fmt=fmt)
        compare({"agg": magg, "vst": mvst}, want, "(f) mirror aggregate", verify=False)
    elif fmt == "affine":
        magg, mvst = ks.multisig_aggregate_pk(rows, c.offs32())
        compare({"agg": magg, "vst": mvst}, want, "(f) mirror aggregate", verify=False)


# ---- (g) ----
def test_g_state_across_calls(eng, ks):
    import torch
    gc = gcs.group_transcripts(3, 20, seed=1250, threads=THREADS)
    gc.case.corrupt(4, 1)
    keys, sk = key_set()
    kc = kcs.pool_transcripts([3, 2, 4], 1251, keys, sk, threads=THREADS)

    def others():
        a = gc.case.args()
        inl = tuple(t.cpu().numpy() for t in eng.multisig_combine(*[dev(x) for x in a[:5]], a[5]))
        with eng.multisig_group(gc.PK) as grp:
            g_out = tuple(t.cpu().numpy() for t in grp.combine(*[dev(x) for x in gc.call_args()]))
        idx, z, R, S, m, offs = kc.args()
        k_out = tuple(t.cpu().numpy() for t in ks.multisig_combine(dev(idx.view(np.int32)), dev(z), dev(R), dev(S), dev(m), offs))
        return inl + g_out + k_out
    before = others()
    first = {}
    for form in FORMS:
        first[form] = run_and_check(form, mix(form), handle_of(form, ks), f"(g) {form} small", oracle=False)
        run_and_check(form, ragged_8193(form), handle_of(form, ks), f"(g) {form} larger: the scratch grows", oracle=False)
        again = run_and_check(form, mix(form), handle_of(form, ks), f"(g) {form} small again", oracle=False)
        for k in ("agg", "st", "tally"):
            assert (first[form][k] == again[k]).all(), (form, k)
    after = others()
    for x, y in zip(before, after):
        assert (x == y).all(), "an existing call's bytes changed"
    mc.check(gc.case, mc.expected(gc.case, THREADS), before[:5], "(g) inline combine beside")
    # the torch route of both mirrors
    c = mix("inline")
    mst, mtally, magg = eng.multisig_verify(dev(c.PK), c.offs32(), dev(c.u), dev(c.R), dev(c.m))
    kcase = mix("keyset")
    kst, ktally, kagg = ks.multisig_verify(dev(kcase.key_idx.view(np.int32)), kcase.offs32(), dev(kcase.u), dev(kcase.R), dev(kcase.m))
    magg2, mvst = eng.multisig_aggregate_pk(dev(c.PK), c.offs32())
    torch.cuda.synchronize()
    assert (mst.cpu().numpy() == first["inline"]["st"]).all() and (magg.cpu().numpy() == first["inline"]["agg"]).all()
    assert mtally.cpu().numpy().tolist() == first["inline"]["tally"].tolist()
    assert (kst.cpu().numpy() == first["keyset"]["st"]).all() and (kagg.cpu().numpy() == first["keyset"]["agg"]).all()
    assert (magg2.cpu().numpy() == first["inline"]["agg"]).all() and (mvst.cpu().numpy() == np.where(c.usable(), 0, 3)).all()
    # two different verification calls queued on two streams without a synchronisation between them: the second waits for the
    # scratch of the first, whose verification stage still reads the normalised R column from it
    x = vc.ext_mix(keys, sk, "inline", threads=THREADS)
    a, b = Call("inline", x.case, ext=x), Call("keyset", mix("keyset"), ks.handle)
    alone = []
    for call in (a, b):
        assert call.launch() == 0
        alone.append(call.read())
    a2, b2 = Call("inline", x.case, ext=x), Call("keyset", mix("keyset"), ks.handle)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        assert a2.launch() == 0
    with torch.cuda.stream(s2):
        assert b2.launch() == 0
    with torch.cuda.stream(s1):
        assert b.launch() == 0                  # and the other order on the first stream again
    torch.cuda.synchronize()
    for call, want in ((a2, alone[0]), (b2, alone[1]), (b, alone[1])):
        got = call.read()
        for k in ("agg", "st", "tally"):
            assert (got[k] == want[k]).all(), ("two streams", k)
    compare(alone[0], vc.expected(x.case, THREADS, x.derived_R), "(g) the extended call alone")


# ---- (h) ----
def test_h_argument_errors(eng, ks):
    import torch
    keys, sk = key_set()
    c = vc.build([[0, 1], [2]], 1260, keys, sk, THREADS)
    calls = [Call(form, c, handle_of(form, ks), verify=v) for form in FORMS for v in (False, True)]
    for call in calls:
        if call.verify or call.form == "inline":
            assert call.launch(fmt=2) == -1, "wire format"
        assert call.launch(agg=None) == -1, "agg_pk = NULL"
        assert call.launch(agg=ctypes.c_void_p(call.agg.data_ptr() + 8)) == -1, "a misaligned agg_pk"
        if call.form == "keyset":
            gone = eng.keyset("single", keys[:3])
            stale = gone.handle
            gone.close()
            for h in (stale, 0, 12345):
                assert call.launch(handle=h) == -1, h
            with eng.multisig_group(keys[:3]) as grp:
                assert call.launch(handle=grp.handle) == -1, "a signer group's handle"
            with eng.keyset("double", keys[:2], keys[2:4]) as dbl:
                assert call.launch(handle=dbl.handle) == -1
                assert b"JJS_SCHEME_SINGLE" in lib().jjs_last_error()
            assert call.launch(keys=ctypes.c_void_p(call.keys.data_ptr() + 2)) == -1, "a misaligned key_idx"
            assert call.launch(keys=None) == -1
        else:
            assert call.launch(keys=ctypes.c_void_p(call.keys.data_ptr() + 4)) == -1, "a misaligned PK"
        assert call.untouched(), "an argument error wrote something"
        # B = 0: nothing but the tally of a verification call, which is zeroed
        assert call.launch(B=0) == 0
        torch.cuda.synchronize()
        assert call.tally.cpu().numpy().tolist() == ([0] * 4 if call.verify else [-6] * 4)
        call.tally.fill_(-6)
        assert call.untouched(), "an empty call wrote something"
    # offsets that do not start at 0, or decrease
    call = calls[1]
    call.offs = np.array([1, 2, 3], np.uint32)
    assert call.launch() == -1
    call.offs = np.array([0, 3, 2], np.uint32)
    assert call.launch() == -1 and call.untouched()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    agg, st, tally = np.full((2, 64), FILL, np.uint8), np.full(2, FILL, np.uint8), np.full(4, 7, np.uint64)
    offs = c.offs32()
    assert lib().jjs_multisig_verify(2, p(c.PK), p(offs), p(c.u), p(c.R), p(c.m), 2, p(agg), p(st), p(tally)) == -1
    assert lib().jjs_multisig_verify(0, p(c.PK), p(offs), p(c.u), p(c.R), p(c.m), 2, None, p(st), p(tally)) == -1
    assert lib().jjs_multisig_verify_keyset(0, 0, p(c.key_idx), p(offs), p(c.u), p(c.R), p(c.m), 2, p(agg), p(st), p(tally)) == -1
    assert lib().jjs_multisig_aggregate_pk_keyset(12345, p(c.key_idx), p(offs), 2, p(agg), p(st)) == -1
    assert (agg == FILL).all() and (st == FILL).all() and (tally == 7).all()
    assert lib().jjs_multisig_verify(0, p(c.PK), p(offs), p(c.u), p(c.R), p(c.m), 0, p(agg), p(st), p(tally)) == 0
    assert (agg == FILL).all() and (st == FILL).all() and (tally == 0).all()
    # and the calls still work
    for call in calls:
        call.offs = c.offs32()
        assert call.launch() == 0
        out = call.read()
        assert out["st"].tolist() == [0, 0] if call.verify else out["vst"].tolist() == [0, 0]


# ---- (i) ----
@pytest.mark.parametrize("form", FORMS)
def test_i_second_trip_of_the_grid_stride_loop(ks, form):
    lanes = lib().jjs_debug_msig_resident_lanes()
    assert lanes > 0
    n = lanes + 64
    c = one_key_vectors(form, n)
    assert c.n == n == c.B
    out = run_and_check(form, c, handle_of(form, ks), f"(i) {form} {n} vectors, resident lanes {lanes}", oracle=False)
    st = out["st"]
    assert (st[:(n // 1024) * 1024].reshape(-1, 1024) == st[:1024]).all() and st[17] == 2 and st[33] == 3 and st[n - 1] == st[(n - 1) % 1024]


# ---- (j) ----
def test_j_known_answers(eng):
    from helpers import to_pt
    k = json.load(open(os.path.join(GOLDEN, "reference_kat.json")))["multisig_kat"]
    PK = np.stack([pt_bytes(o.decompress(bytes.fromhex(x))) for x in k["public_keys"]])
    sig = bytes.fromhex(k["signature"])
    u = np.frombuffer(sig[:32], np.uint8).reshape(1, 32)
    R = pt_bytes(o.decompress(sig[32:])).reshape(1, 64)
    m = np.frombuffer(o.le32(k["message"]), np.uint8).reshape(1, 32)
    st, tally, agg = eng.multisig_verify(PK, [0, len(PK)], u, R, m)
    assert o.compress(to_pt(agg[0])).hex() == k["aggregate_public_key"] and st.tolist() == [0] and tally.tolist() == [1, 0, 0, 0]
    agg2, vst = eng.multisig_aggregate_pk(PK, [0, len(PK)])
    assert (agg2 == agg).all() and vst.tolist() == [0]
    z = np.load(os.path.join(GOLDEN, "multisig_valid_transcripts.npz"))
    per, B = int(z["participants"]), len(z["m"])
    offs = np.arange(B + 1, dtype=np.uint32) * per
    st, tally, agg = eng.multisig_verify(dev(z["PK"]), offs, dev(z["sig_u"]), dev(z["sig_R"]), dev(z["m"]))
    assert (agg.cpu().numpy() == z["agg_pk"]).all() and not st.cpu().numpy().any() and tally.cpu().numpy().tolist() == [B, 0, 0, 0]
    flipped = z["sig_u"].copy()
    flipped[:, 0] ^= 1
    st, tally, agg = eng.multisig_verify(dev(z["PK"]), offs, dev(flipped), dev(z["sig_R"]), dev(z["m"]))
    assert (agg.cpu().numpy() == z["agg_pk"]).all() and (st.cpu().numpy() == 2).all() and tally.cpu().numpy().tolist() == [0, 0, B, 0]

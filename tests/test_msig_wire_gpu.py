"""The wire forms of the multisignature calls on the device (jjs_multisig_*_wire*, jjs_msig_group_*_wire*).  The contract is
byte equality with the affine twin on derived columns: every wire _dev call is compared, every output, with the affine _dev call
on columns derived ON THE DEVICE -- `Engine.decompress` output with the ok == 0 rows overwritten by 0xFF -- which are themselves
cross-checked against the derived columns msig_wire_cases.py computes in Python integers.  Then the blocking host forms against
the _dev forms, groups from wire keys against groups from affine keys, the key-set forms, the reference's multisignature known
answer from its wire bytes, and the argument errors.  Timing is asserted nowhere."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import jjs_oracle as o
import msig_group_cases as gcs
import msig_keyset_cases as kcs
import msig_wire_cases as wc
import multisig_cases as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = 16
GROUP_NAMES = ("share_status", "sig_u", "sig_R", "transcript_status")
VERIFY_NAMES = ("status", "tally", "agg_pk")


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


def derived_on_device(eng, wire, want=None):
    """The derived column of the contract, made by the engine's own decoder: jjs_decompress_dev, 0xFF where ok == 0.  want: the
    same column from Python integers."""
    import torch
    pts, ok = eng.decompress(dev(wire))
    pts = pts.clone()
    pts[ok == 0] = 0xFF
    torch.cuda.synchronize()
    got = pts.cpu().numpy()
    if want is None:
        want = wc.derive_column(wire)
    assert (got == want).all(), "jjs_decompress_dev against jjs_oracle.decompress"
    return pts


@functools.lru_cache(None)
def shape(name):
    """The inline shapes: a WireCase each, built once."""
    if name == "210 ragged, planted":
        x = wc.WireCase(mc.filler(210, seed=31, top=5, threads=THREADS))
        wc.plant_everywhere(x, boundary=x.T // 2)
    elif name == "257 participants":            # crosses the boundary of the tag table
        x = wc.WireCase(mc.valid_transcripts([mc.TABLE_PARTICIPANTS + 1], seed=1601, threads=THREADS))
        x.plant(0, 0, "PK", "identity"); x.plant(0, 128, "R", "v=q-1 signed"); x.plant(0, 256, "S", "order 4 +")
    elif name == "1 participant":
        x = wc.WireCase(mc.valid_transcripts([1], seed=1602, threads=THREADS))
    elif name == "1 participant, undecodable":
        x = wc.WireCase(mc.valid_transcripts([1], seed=1602, threads=THREADS))
        x.plant(0, 0, "S", "0xFF")
    elif name == "an empty transcript between two":
        x = wc.WireCase(mc.valid_transcripts([3, 0, 2], seed=1603, threads=THREADS))
        x.plant(2, 0, "R", "non-residue"); x.plant(0, 1, "PK", "odd u")
    else:
        assert name == "B = 1"
        x = wc.WireCase(mc.valid_transcripts([5], seed=1604, threads=THREADS))
        x.plant(0, 4, "PK", "v=1 signed")
    x.check_derived()
    return x


SHAPES = ("210 ragged, planted", "257 participants", "1 participant", "1 participant, undecodable", "an empty transcript between two", "B = 1")


def derived_args(eng, x):
    d = x.derived.dirty
    return [dev(d["z"])] + [derived_on_device(eng, x.wire[c], d[c]) for c in wc.POINT_COLS] + [dev(d["m"])]


def signatures(x, combined):
    """One aggregate signature per transcript as wire bytes, u || R: what the combine call made of it (zeros where it made
    none: v = 0 decodes), the last one with an R that does not decode."""
    _, _, su, sr, _ = combined
    sig = wc.sig_rows(su, wc.compress_column(sr))
    sig[-1, 32:] = np.frombuffer(wc.encoding("v=q"), np.uint8)
    return sig


# ---- the inline _dev calls against their affine twins ----
@pytest.mark.parametrize("name", SHAPES)
def test_inline_calls_against_their_affine_twins(eng, name):
    x = shape(name)
    a = x.args()
    offs = a[5]
    ins = derived_args(eng, x)
    # combine
    got = host(eng.multisig_combine_wire(*[dev(c) for c in a[:5]], offs))
    want = host(eng.multisig_combine(*ins, offs))
    same(got, want, name + ": combine")
    for t, j, _, kind in x.plants:
        if kind in wc.UNDECODABLE:
            assert got[0][x.derived.row(t, j)] == 3 and got[4][t] != 0 and not got[2][t].any() and not got[3][t].any(), (name, t, j, kind)
    if not any(kind in wc.UNDECODABLE for *_, kind in x.plants):
        mc.check(x.derived, mc.expected(x.derived, THREADS), got, name)
    # aggregate_pk
    agg = host(eng.multisig_aggregate_pk_wire(dev(x.wire["PK"]), offs))
    same(agg, host(eng.multisig_aggregate_pk(ins[1], offs)), name + ": aggregate_pk", ("agg_pk", "vec_status"))
    for t, j, col, kind in x.plants:
        if col == "PK" and kind in wc.UNDECODABLE:
            assert agg[1][t] == 3 and not agg[0][t].any(), (name, t)
    # verify
    sig = signatures(x, got)
    r = derived_on_device(eng, np.ascontiguousarray(sig[:, 32:]))
    v = host(eng.multisig_verify_wire(dev(x.wire["PK"]), offs, dev(sig), ins[4]))
    same(v, host(eng.multisig_verify(ins[1], offs, dev(np.ascontiguousarray(sig[:, :32])), r, ins[4])), name + ": verify", VERIFY_NAMES)
    assert int(v[1].sum()) == x.T and v[0][-1] == 3, (name, "the tally sums to B; an undecodable R is status 3")
    ok = (got[4] == 0)
    ok[-1] = False
    assert (v[0][ok] == 0).all(), (name, "the signatures the combine call made verify")
    print(f"wire {name}: shares={x.n} T={x.T} planted={len(x.plants)} combined={int((got[4] == 0).sum())} verified={int((v[0] == 0).sum())}")


# ---- the blocking host calls against the _dev calls ----
def test_host_forms_against_device_forms(eng):
    x = shape("210 ragged, planted")
    a = x.args()
    want = host(eng.multisig_combine_wire(*[dev(c) for c in a[:5]], a[5]))
    same(eng.multisig_combine_wire(*a), want, "host combine")
    agg = host(eng.multisig_aggregate_pk_wire(dev(x.wire["PK"]), a[5]))
    same(eng.multisig_aggregate_pk_wire(x.wire["PK"], a[5]), agg, "host aggregate_pk", ("agg_pk", "vec_status"))
    sig = signatures(x, want)
    v = host(eng.multisig_verify_wire(dev(x.wire["PK"]), a[5], dev(sig), dev(a[4])))
    same(eng.multisig_verify_wire(x.wire["PK"], a[5], sig, a[4]), v, "host verify", VERIFY_NAMES)
    # unaligned host pointers, and no transcript_status
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    odd = []
    for c in a[:5]:
        buf = np.zeros(c.size + 1, np.uint8)
        buf[1:] = c.reshape(-1)
        odd.append(buf[1:].reshape(c.shape))
    p = lambda t: t.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st, agg2, su, sr = np.full(x.n, 0xA5, np.uint8), np.full((x.T, 64), 0xA5, np.uint8), np.full((x.T, 32), 0xA5, np.uint8), np.full((x.T, 64), 0xA5, np.uint8)
    assert lib.jjs_multisig_combine_wire(*[p(c) for c in odd], p(a[5]), x.T, p(st), None, p(agg2), p(su), p(sr)) == 0, lib.jjs_last_error()
    same((st, agg2, su, sr), want[:4], "host wire, odd addresses", mc.OUTPUTS[:4])


# ---- signer groups ----
@functools.lru_cache(None)
def group_case(n):
    return gcs.group_transcripts(n, 64, seed=850 + n, threads=THREADS)


@pytest.mark.parametrize("n", [1, 8])
def test_group_calls(eng, n):
    """The group from wire keys is the group from the affine keys; combine_wire with planted R and S on both sides of the
    lane-mapping boundary (B = 63, 64)."""
    full = group_case(n)
    pk_w = wc.compress_column(full.PK)
    with eng.multisig_group_wire(pk_w) as gw, eng.multisig_group(full.PK) as ga:
        assert (gw.aggregate_pk == ga.aggregate_pk).all() and gw.participants == n
        for B in (1, 63, 64):
            gc = full.slice(0, B)
            x = wc.WireCase(gc.case)
            z, m = dev(gc.case.dirty["z"]), dev(gc.case.dirty["m"])
            got = host(gw.combine_wire(z, dev(x.wire["R"]), dev(x.wire["S"]), m))
            want = host(ga.combine(z, dev(gc.case.dirty["R"]), dev(gc.case.dirty["S"]), m))
            same(got, want, f"group n={n} B={B} clean", GROUP_NAMES)
            same(got, host(gw.combine(z, dev(gc.case.dirty["R"]), dev(gc.case.dirty["S"]), m)), f"wire group, affine call n={n} B={B}", GROUP_NAMES)
            mc.check(gc.case, mc.expected(gc.case, THREADS), gcs.as_inline_outputs(gc, gw.aggregate_pk, got), f"group n={n} B={B}")
            assert (got[3] == 0).all()
            x.plant(B - 1, n - 1, "R", "non-residue"); x.plant(0, 0, "S", "v=q-1 signed")
            if n > 2:
                x.plant(0, 1, "R", "order 4 -")
            r, s = derived_on_device(eng, x.wire["R"], x.derived.dirty["R"]), derived_on_device(eng, x.wire["S"], x.derived.dirty["S"])
            got = host(gw.combine_wire(z, dev(x.wire["R"]), dev(x.wire["S"]), m))
            same(got, host(ga.combine(z, r, s, m)), f"group n={n} B={B} planted", GROUP_NAMES)
            assert got[0][0] == 3 and got[0][-1] == 3 and got[3][0] == 3 and got[3][B - 1] != 0 and not got[1][0].any()
        # the blocking form
        d = x.derived.dirty
        same(gw.combine_wire(d["z"], x.wire["R"], x.wire["S"], d["m"]), got, f"group n={n} host", GROUP_NAMES)


@pytest.mark.parametrize("kind", wc.UNDECODABLE)
def test_a_registration_with_an_undecodable_key_is_refused(eng, kind):
    from jubjub_schnorr_amd import _ffi
    pk_w = wc.compress_column(group_case(8).PK)
    for j in (0, 7):
        spoilt = pk_w.copy()
        spoilt[j] = np.frombuffer(wc.encoding(kind), np.uint8)
        with pytest.raises(_ffi.JjsError, match="code -1"):
            eng.multisig_group_wire(spoilt)
    edge = pk_w.copy()
    edge[3] = np.frombuffer(wc.encoding("order 2"), np.uint8)           # decodable: registered, as from its affine form
    with eng.multisig_group_wire(edge) as gw, eng.multisig_group(wc.derive_column(edge)) as ga:
        assert (gw.aggregate_pk == ga.aggregate_pk).all()


# ---- the key-set forms ----
def test_key_set_forms(eng):
    keys, sk = kcs.key_set()
    kc = kcs.pool_transcripts([2, 3, 1, 8, 5], 1610, keys, sk, threads=THREADS)
    kc.case.corrupt(3, 2)
    x = wc.WireCase(kc.case)
    idx = dev(kc.key_idx.view(np.int32))
    offs = kc.case.offsets.astype(np.uint32)
    d = x.derived.dirty
    z, m = dev(d["z"]), dev(d["m"])
    with eng.keyset("single", keys) as ks:
        clean = host(ks.multisig_combine_wire(idx, z, dev(x.wire["R"]), dev(x.wire["S"]), m, offs))
        same(clean, host(ks.multisig_combine(idx, z, dev(d["R"]), dev(d["S"]), m, offs)), "key set, usable rows")
        assert clean[4].tolist() == [0, 0, 0, 4, 0]
        mc.check(kc.case, kcs.expected(kc, THREADS), clean, "key set, wire")
        x.plant(1, 0, "R", "0xFF"); x.plant(4, 2, "S", "identity")
        x.check_derived()
        r, s = derived_on_device(eng, x.wire["R"], d["R"]), derived_on_device(eng, x.wire["S"], d["S"])
        got = host(ks.multisig_combine_wire(idx, z, dev(x.wire["R"]), dev(x.wire["S"]), m, offs))
        same(got, host(ks.multisig_combine(idx, z, r, s, m, offs)), "key set, planted")
        assert got[4].tolist() == [0, 3, 0, 4, got[4][4]] and got[4][4] not in (0, 3), "status 3 for the planted transcript only"
        assert got[0][x.derived.row(1, 0)] == 3 and not got[2][1].any() and not got[3][1].any()
        same(ks.multisig_combine_wire(kc.key_idx, d["z"], x.wire["R"], x.wire["S"], d["m"], offs), got, "key set, host form")
        # the verifier's call by key set: the signature column alone is wire
        sig = signatures(x, clean)
        rr = derived_on_device(eng, np.ascontiguousarray(sig[:, 32:]))
        v = host(ks.multisig_verify_wire(idx, offs, dev(sig), m))
        same(v, host(ks.multisig_verify(idx, offs, dev(np.ascontiguousarray(sig[:, :32])), rr, m)), "key set verify", VERIFY_NAMES)
        assert v[0].tolist()[:3] == [0, 0, 0] and v[0][4] == 3 and int(v[1].sum()) == kc.T
        same(ks.multisig_verify_wire(kc.key_idx, offs, sig, d["m"]), v, "key set verify, host form", VERIFY_NAMES)


# ---- the reference's known answer ----
def test_the_reference_known_answer_from_its_wire_bytes(eng):
    with open(os.path.join(HERE, "golden", "reference_kat.json")) as f:
        k = json.load(f)["multisig_kat"]
    col = lambda xs: np.frombuffer(b"".join(bytes.fromhex(x) for x in xs), np.uint8).reshape(len(xs), 32).copy()  # noqa: E731
    pk_w, r_w, s_w, z = col(k["public_keys"]), col(k["r_points"]), col(k["s_points"]), col(k["individual_shares"])
    m = np.frombuffer(o.le32(k["message"]), np.uint8).reshape(1, 32).copy()
    # the combiner
    st, agg, su, sr, ts = host(eng.multisig_combine_wire(dev(z), dev(pk_w), dev(r_w), dev(s_w), dev(m), [0, 3]))
    assert st.tolist() == [0, 0, 0] and ts.tolist() == [0]
    assert wc.compress_column(agg)[0].tobytes().hex() == k["aggregate_public_key"]
    assert (su[0].tobytes() + wc.compress_column(sr)[0].tobytes()).hex() == k["signature"]
    wire_out = host((eng.compress(dev(agg)), eng.compress(dev(sr))))
    assert wire_out[0][0].tobytes().hex() == k["aggregate_public_key"] and wire_out[1][0].tobytes().hex() == k["signature"][64:]
    # the verifier: the signature, one bit of u flipped, an R that does not decode
    sig = np.tile(np.frombuffer(bytes.fromhex(k["signature"]), np.uint8), (3, 1)).copy()
    sig[1, 0] ^= 1
    sig[2, 32:] = np.frombuffer(wc.encoding("v=1 signed"), np.uint8)
    status, tally, agg3 = host(eng.multisig_verify_wire(dev(np.tile(pk_w, (3, 1))), [0, 3, 6, 9], dev(sig), dev(np.tile(m, (3, 1)))))
    assert status.tolist() == [0, 2, 3] and tally.tolist() == [1, 0, 1, 1] and int(tally.sum()) == 3
    assert (agg3 == agg[0]).all()
    agg1, vst = host(eng.multisig_aggregate_pk_wire(dev(pk_w), [0, 3]))
    assert vst.tolist() == [0] and (agg1 == agg).all()


# ---- argument errors ----
def test_argument_errors(eng):
    import torch
    from jubjub_schnorr_amd import _ffi
    lib = _ffi.lib()
    x = wc.WireCase(mc.valid_transcripts([2, 3], seed=921, threads=THREADS))
    a = x.args()
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    q = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = [np.zeros(x.n, np.uint8), np.zeros(x.T, np.uint8), np.zeros((x.T, 64), np.uint8), np.zeros((x.T, 32), np.uint8), np.zeros((x.T, 64), np.uint8)]
    cols = [p(c) for c in a[:5]]
    host_call = lambda cols, offs=a[5], T=x.T: lib.jjs_multisig_combine_wire(*cols, p(offs), T, *[p(v) for v in outs])  # noqa: E731
    assert host_call(cols) == 0 and outs[1].tolist() == [0, 0]
    for k in range(5):
        assert host_call(cols[:k] + [None] + cols[k + 1:]) == -1, k
    assert host_call(cols, np.array([0, 3, 2], np.uint32)) == -1 and host_call(cols, np.array([1, 2, 5], np.uint32)) == -1, "offsets"
    assert host_call(cols, T=0) == 0
    # the calls that take a format still refuse the wire format: these entry points are the wire form
    assert lib.jjs_multisig_combine(2, *cols, p(a[5]), x.T, *[p(v) for v in outs]) == -1
    assert lib.jjs_multisig_aggregate_pk(2, cols[1], p(a[5]), x.T, p(outs[2]), p(outs[1])) == -1
    ins = [dev(c) for c in a[:5]]
    douts = [dev(v) for v in outs]
    dev_call = lambda din, offs=a[5]: lib.jjs_multisig_combine_wire_dev(*din, p(offs), x.T, *[q(t) for t in douts], s)  # noqa: E731
    assert dev_call([q(t) for t in ins]) == 0
    assert dev_call([q(t) for t in ins], np.array([0, 3, 2], np.uint32)) == -1, "decreasing offsets"
    for k in range(1, 4):
        din = [q(t) for t in ins]
        din[k] = None
        assert dev_call(din) == -1, k
        din[k] = ctypes.c_void_p(ins[k].data_ptr() + 8)
        assert dev_call(din) == -1, ("misaligned", k)
    # the verifier's calls: sig_w NULL and misaligned
    sig, tally = dev(np.zeros((x.T, 64), np.uint8)), torch.zeros(4, dtype=torch.int64, device="cuda")
    vcall = lambda pk, sg: lib.jjs_multisig_verify_wire_dev(pk, p(a[5]), sg, q(ins[4]), x.T, q(douts[2]), q(douts[1]), q(tally), s)  # noqa: E731
    assert vcall(q(ins[1]), q(sig)) == 0
    assert vcall(q(ins[1]), None) == -1 and vcall(None, q(sig)) == -1
    assert vcall(q(ins[1]), ctypes.c_void_p(sig.data_ptr() + 8)) == -1 and vcall(ctypes.c_void_p(ins[1].data_ptr() + 4), q(sig)) == -1
    assert lib.jjs_multisig_aggregate_pk_wire_dev(None, p(a[5]), x.T, q(douts[2]), q(douts[1]), s) == -1
    # a stale group handle
    pk_w = wc.compress_column(group_case(8).PK)
    g = eng.multisig_group_wire(pk_w)
    h = g.handle
    gz, gm, gr = dev(np.zeros((8, 32), np.uint8)), dev(np.zeros((1, 32), np.uint8)), dev(np.full((8, 32), 0xFF, np.uint8))
    gout = [dev(np.zeros(8, np.uint8)), dev(np.zeros(1, np.uint8)), dev(np.zeros((1, 32), np.uint8)), dev(np.zeros((1, 64), np.uint8))]
    dargs = lambda B: (q(gz), q(gr), q(gr), q(gm), B, *[q(t) for t in gout], s)  # noqa: E731
    hz, hr, hm = np.zeros((8, 32), np.uint8), np.full((8, 32), 0xFF, np.uint8), np.zeros((1, 32), np.uint8)
    hout = [np.zeros(8, np.uint8), np.zeros(1, np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)]
    hargs = lambda B: (p(hz), p(hr), p(hr), p(hm), B, *[p(v) for v in hout])  # noqa: E731
    assert lib.jjs_msig_group_combine_wire_dev(h, *dargs(1)) == 0 and lib.jjs_msig_group_combine_wire(h, *hargs(1)) == 0
    torch.cuda.synchronize()
    assert hout[0].tolist() == [3] * 8 and gout[0].cpu().numpy().tolist() == [3] * 8, "undecodable everywhere: status 3"
    assert lib.jjs_msig_group_combine_wire_dev(h, *dargs(1 << 29)) == -1 and lib.jjs_msig_group_combine_wire(h, *hargs(1 << 29)) == -1
    assert lib.jjs_msig_group_combine(h, 2, *hargs(1)) == -1
    g.close()
    assert lib.jjs_msig_group_combine_wire_dev(h, *dargs(1)) == -1 and lib.jjs_msig_group_combine_wire(h, *hargs(1)) == -1
    assert lib.jjs_msig_group_combine_wire(h, *hargs(0)) == -1, "a stale handle is refused before the empty call returns"
    # a key set of another scheme, and a stale one
    keys, _ = kcs.key_set()
    idx = dev(np.array([0, 1, 2, 3, 4], np.int32))
    kargs = lambda: (q(idx), q(ins[0]), q(ins[2]), q(ins[3]), q(ins[4]), p(a[5]), x.T, *[q(t) for t in douts], s)  # noqa: E731
    vargs = lambda: (q(idx), p(a[5]), q(sig), q(ins[4]), x.T, q(douts[2]), q(douts[1]), q(tally), s)  # noqa: E731
    with eng.keyset("double", keys[:2], keys[2:4]) as dbl:
        assert lib.jjs_multisig_combine_keyset_wire_dev(dbl.handle, *kargs()) == -1
        assert b"JJS_SCHEME_SINGLE" in lib.jjs_last_error()
        assert lib.jjs_multisig_verify_keyset_wire_dev(dbl.handle, *vargs()) == -1
    ks = eng.keyset("single", keys)
    assert lib.jjs_multisig_combine_keyset_wire_dev(ks.handle, *kargs()) == 0 and lib.jjs_multisig_verify_keyset_wire_dev(ks.handle, *vargs()) == 0
    assert lib.jjs_multisig_combine_keyset_dev(ks.handle, 2, *kargs()) == -1
    stale = ks.handle
    ks.close()
    assert lib.jjs_multisig_combine_keyset_wire_dev(stale, *kargs()) == -1 and lib.jjs_multisig_verify_keyset_wire_dev(stale, *vargs()) == -1
    torch.cuda.synchronize()

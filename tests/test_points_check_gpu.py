"""`is_valid` alone on the MI355X (jjs_keys_check(_dev), jjs_signatures_check(_dev)): the case lists of points_check_cases.py
through the resident and the host form of both calls, for every scheme and format, without outputs (extended points: the
projective tests, no inversion) and with them, at the wave, block and two-lanes-per-item boundaries, against the oracle; keys also
against jjs_keyset_create's key_status, affine points against jjs_debug_point_flags_dev, wire outputs against
jjs_decompress_dev."""
import ctypes

import numpy as np
import pytest

import points_check_cases as pc

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def call(eng, kind, scheme, fmt, cols, want_points, resident):
    fn = eng.keys_check if kind == "keys" else eng.signatures_check
    cols = [c for c in cols if c is not None]
    if not resident:
        r = fn(scheme, *cols, fmt=fmt, want_points=want_points)
        return (r[0], r[1], list(r[2]) if want_points else [])
    import torch
    r = fn(scheme, *[dev(c) for c in cols], fmt=fmt, want_points=want_points)
    torch.cuda.synchronize()
    return (r[0].cpu().numpy(), r[1].cpu().numpy(), [a.cpu().numpy() for a in r[2]] if want_points else [])


def compare(got, want, what):
    st, tally, outs = got
    bad = np.where(st != want["status"])[0]
    assert len(bad) == 0, (what, bad[:8], st[bad[:8]], want["status"][bad[:8]])
    assert [int(x) for x in tally] == want["tally"].tolist(), what
    for j, (g, w) in enumerate(zip(outs, [a for a in want["outs"] if a is not None])):
        rows = np.where((g != w).any(1))[0]
        assert len(rows) == 0, (what, "output", j, rows[:8], want["status"][rows[:8]])


@pytest.mark.parametrize("kind,scheme,fmt", pc.ALL)
def test_against_the_oracle(eng, kind, scheme, fmt):
    case = pc.build(kind, scheme, fmt)
    for n in SIZES + (case["n"],):
        for at_end in (True, False):
            want = pc.padded(case, n, at_end)
            for want_points in (False, True):
                for resident in (True, False):
                    compare(call(eng, kind, scheme, fmt, want["cols"], want_points, resident), want,
                            (kind, scheme, fmt, n, at_end, want_points, resident))


@pytest.mark.parametrize("fmt", list(pc.FORMATS))
@pytest.mark.parametrize("scheme", list(pc.SCHEMES))
def test_keys_get_the_key_status_of_a_key_set(eng, scheme, fmt):
    case = pc.build("keys", scheme, fmt)
    st, _, _ = call(eng, "keys", scheme, fmt, case["cols"], False, True)
    with eng.keyset(scheme, case["cols"][0], case["cols"][1], fmt=fmt) as ks:
        np.testing.assert_array_equal(st, ks.key_status)
    np.testing.assert_array_equal(st, case["status"])


def test_affine_points_against_the_debug_flags(eng):
    """bits 0-2 of jjs_debug_point_flags_dev: on the curve, torsion-free or the identity, the identity"""
    import torch
    rows = np.stack([r for r, _, _ in pc.point_cases("affine")])
    want = np.array([s for _, s, _ in pc.point_cases("affine")], np.uint8)
    flags = eng.debug_point_flags(dev(rows))
    st, _, _ = call(eng, "keys", "single", "affine", [rows, None], False, True)
    torch.cuda.synchronize()
    flags = flags.cpu().numpy() & 7
    in_range = want != 3
    np.testing.assert_array_equal(st[in_range], np.where(flags[in_range] == 3, 0, 1))
    np.testing.assert_array_equal(st, want)
    # ... and as the R column of signatures and the second column of two-point keys
    u = np.zeros((len(rows), 32), np.uint8)
    st, _, _ = call(eng, "signatures", "vargen", "affine", [u, rows, None], False, True)
    np.testing.assert_array_equal(st, want)
    good = np.tile(rows[0], (len(rows), 1))
    st, _, _ = call(eng, "keys", "vargen", "affine", [good, rows], False, True)
    np.testing.assert_array_equal(st, want)


def test_wire_outputs_against_decompress(eng):
    import torch
    enc = np.stack([r for r, _, _ in pc.point_cases("wire")])
    affine, ok = eng.decompress(dev(enc))
    st, _, outs = call(eng, "keys", "single", "wire", [enc, None], True, True)
    torch.cuda.synchronize()
    affine, ok = affine.cpu().numpy(), ok.cpu().numpy()
    np.testing.assert_array_equal(st == 3, ok == 0)
    np.testing.assert_array_equal(outs[0][ok == 1], affine[ok == 1])
    assert not outs[0][ok == 0].any()


def test_tally_across_many_blocks(eng):
    """2^16 + 1 keys drawn from the valid and the torsion-shifted points"""
    import torch
    pts = [(r, s) for i, (r, s, _) in enumerate(pc.point_cases("affine")) if i < 16 or 24 <= i < 31]      # 16 valid, 7 of them plus k T8
    assert sorted({s for _, s in pts}) == [0, 1]
    rows, sts = np.stack([r for r, _ in pts]), np.array([s for _, s in pts], np.uint8)
    pick = np.random.default_rng(65537).integers(0, len(pts), (1 << 16) + 1)
    keys, want = np.ascontiguousarray(rows[pick]), sts[pick]
    st, tally = eng.keys_check("single", dev(keys))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st.cpu().numpy(), want)
    assert tally.cpu().numpy().tolist() == [int((want == k).sum()) for k in range(4)]
    pair = np.ascontiguousarray(keys[::-1])
    st, tally = eng.keys_check("double", dev(keys), dev(pair))
    torch.cuda.synchronize()
    both = np.maximum(want, want[::-1])
    np.testing.assert_array_equal(st.cpu().numpy(), both)
    assert tally.cpu().numpy().tolist() == [int((both == k).sum()) for k in range(4)]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_empty_calls_null_outputs_and_argument_errors(eng):
    import torch
    lib = eng._lib
    stream = eng._stream()
    case = pc.build("keys", "single", "affine")
    keys, n = dev(case["cols"][0]), case["n"]
    sig = pc.build("signatures", "double", "affine")
    s = [dev(c) for c in sig["cols"]]
    # n == 0: 0, a zero tally and nothing else written
    tally = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    status = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((64, 64), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.jjs_keys_check_dev(0, 0, _ptr(keys), None, 0, _ptr(status), _ptr(tally), _ptr(out), None, stream) == 0
    torch.cuda.synchronize()
    assert tally.cpu().tolist() == [0] * 4 and (status.cpu() == 0xA5).all() and (out.cpu() == 0xA5).all()
    tally.fill_(7)
    assert lib.jjs_signatures_check_dev(1, 0, None, None, None, 0, None, _ptr(tally), None, None, None, stream) == 0
    torch.cuda.synchronize()
    assert tally.cpu().tolist() == [0] * 4
    ht = np.full(4, 7, np.uint64)
    assert lib.jjs_keys_check(0, 2, None, None, 0, None, ht.ctypes.data_as(ctypes.c_void_p), None, None) == 0 and ht.tolist() == [0] * 4
    assert lib.jjs_signatures_check(2, 1, None, None, None, 0, None, ht.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
    assert lib.jjs_keys_check_dev(0, 0, None, None, 0, None, None, None, None, stream) == 0
    # a NULL tally, a NULL status
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.jjs_keys_check_dev(0, 0, _ptr(keys), None, n, _ptr(status), None, None, None, stream) == 0
    tally.fill_(7)
    assert lib.jjs_keys_check_dev(0, 0, _ptr(keys), None, n, None, _ptr(tally), None, None, stream) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), case["status"])
    assert tally.cpu().tolist() == case["tally"].tolist()
    hs = np.empty(sig["n"], np.uint8)
    hp = [c.ctypes.data_as(ctypes.c_void_p) for c in sig["cols"]]
    assert lib.jjs_signatures_check(1, 0, *hp, sig["n"], hs.ctypes.data_as(ctypes.c_void_p), None, None, None, None) == 0
    np.testing.assert_array_equal(hs, sig["status"])
    assert lib.jjs_signatures_check(1, 0, *hp, sig["n"], None, ht.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
    assert ht.tolist() == sig["tally"].tolist()
    # argument errors
    for scheme, fmt in ((3, 0), (-1, 0), (0, 3), (0, -1)):
        assert lib.jjs_keys_check_dev(scheme, fmt, _ptr(keys), None, n, None, _ptr(tally), None, None, stream) == -1
        assert lib.jjs_keys_check_dev(scheme, fmt, _ptr(keys), None, 0, None, _ptr(tally), None, None, stream) == -1
        assert lib.jjs_signatures_check(scheme, fmt, *hp, sig["n"], None, None, None, None, None) == -1
    assert lib.jjs_keys_check_dev(0, 0, None, None, n, None, _ptr(tally), None, None, stream) == -1                  # K0 missing
    assert lib.jjs_keys_check_dev(1, 0, _ptr(keys), None, n, None, _ptr(tally), None, None, stream) == -1            # K1 missing
    assert lib.jjs_keys_check_dev(0, 0, _ptr(keys), _ptr(keys), n, None, _ptr(tally), None, None, stream) == -1      # K1 not taken
    assert lib.jjs_keys_check_dev(1, 2, _ptr(keys), _ptr(keys), n, None, _ptr(tally), None, None, stream) == -1      # wire: K0 alone
    assert lib.jjs_keys_check_dev(0, 0, _ptr(keys), None, n, None, _ptr(tally), None, _ptr(out), stream) == -1       # no A1 for single
    assert lib.jjs_keys_check_dev(0, 0, ctypes.c_void_p(keys.data_ptr() + 4), None, n - 1, None, _ptr(tally), None, None, stream) == -1
    assert lib.jjs_signatures_check_dev(0, 0, _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), n, None, _ptr(tally), None, None, None, stream) == -1   # R' for single
    assert lib.jjs_signatures_check_dev(1, 0, _ptr(s[0]), _ptr(s[1]), None, n, None, _ptr(tally), None, None, None, stream) == -1         # R' missing
    assert lib.jjs_signatures_check_dev(1, 2, _ptr(s[0]), _ptr(s[1]), None, n, None, _ptr(tally), None, None, None, stream) == -1         # wire: s0 alone
    assert lib.jjs_signatures_check_dev(2, 0, _ptr(s[0]), _ptr(s[1]), None, n, None, _ptr(tally), None, None, _ptr(out), stream) == -1    # no R' output
    assert lib.jjs_keys_check(1, 0, case["cols"][0].ctypes.data_as(ctypes.c_void_p), None, n, None, None, None, None) == -1
    torch.cuda.synchronize()


def test_the_reference_shaped_types(eng):
    from jubjub_schnorr_amd.api import PublicKey, PublicKeyDouble, PublicKeyVarGen, Signature, SignatureDouble, SignatureVarGen
    pts = pc.point_cases("affine")
    rows, sts = [r.tobytes() for r, _, _ in pts], [s for _, s, _ in pts]
    good = rows[0]
    u = (5).to_bytes(32, "little")
    want = np.array([s == 0 for s in sts])
    np.testing.assert_array_equal(PublicKey.is_valid_batch([PublicKey(r) for r in rows]), want)
    np.testing.assert_array_equal(PublicKeyDouble.is_valid_batch([PublicKeyDouble(good, r) for r in rows]), want)
    np.testing.assert_array_equal(PublicKeyVarGen.is_valid_batch([PublicKeyVarGen(r, good) for r in rows]), want)
    np.testing.assert_array_equal(Signature.is_valid_batch([Signature(u, r) for r in rows]), want)
    np.testing.assert_array_equal(SignatureDouble.is_valid_batch([SignatureDouble(u, r, good) for r in rows]), want)
    np.testing.assert_array_equal(SignatureVarGen.is_valid_batch([SignatureVarGen(u, r) for r in rows]), want)
    assert PublicKey(good).is_valid() and not PublicKey(rows[16]).is_valid()          # rows[16]: the identity
    assert SignatureDouble(u, good, good).is_valid() and not SignatureDouble(bytes([0xFF] * 32), good, good).is_valid()
    assert len(PublicKey.is_valid_batch([])) == 0

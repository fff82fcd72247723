"""jjs_sign_vargen_pt(_dev) and jjs_public_keys_vargen(_dev) on the device, through the C ABI with every output prefilled with 0xA5.
Expected values: the reference's own bytes, the oracle's (sign_vargen_pt_cases.py), and jjs_sign_vargen_dev, the signer that takes
the generator as a scalar, which must give the same bytes for Gen = gen_scalar * G.  Every comparison is byte for byte.  Then
sign_vargen_child.py forces the shared-generator route (profiling build)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import jjs_oracle as o
import sign_vargen_pt_cases as vc
from helpers import to_extended, to_pt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xA5


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


def _filled(rows, width=None):
    import torch
    shape = (max(rows, 1),) if width is None else (max(rows, 1), width)
    return torch.full(shape, FILL, dtype=torch.uint8, device="cuda")[:rows]


def sign_dev(fmt, sk, Gen, rnd, m, want_pk=True, want_gen=True, written=True):
    """jjs_sign_vargen_pt_dev with prefilled outputs -> numpy (u, R, PK, Gen_out, status)."""
    import torch
    n, ng = len(sk), len(Gen)
    cols = [dev(x) for x in (sk, Gen, rnd, m)]
    u, R, PK, G_out, st = _filled(n, 32), _filled(n, 64), _filled(n, 64) if want_pk else None, _filled(ng, 64) if want_gen else None, _filled(n)
    rc = lib().jjs_sign_vargen_pt_dev(vc.FORMAT_CODE[fmt], _ptr(cols[0]), _ptr(cols[1]), ng, _ptr(cols[2]), _ptr(cols[3]), n, _ptr(u), _ptr(R), _ptr(PK),
                                      _ptr(G_out), _ptr(st), _stream())
    assert rc == 0, lib().jjs_last_error()
    torch.cuda.synchronize()
    out = [x.cpu().numpy() if x is not None else None for x in (u, R, PK, G_out, st)]
    if written:
        assert not (out[0] == FILL).all(1).any() and not (out[1] == FILL).all(1).any() and not (out[4] == FILL).any(), "an output row was not written"
    return out


def derive_dev(fmt, sk, Gen):
    import torch
    n, ng = len(sk), len(Gen)
    cols = [dev(sk), dev(Gen)]
    PK, G_out, st = _filled(n, 64), _filled(ng, 64), _filled(n)
    rc = lib().jjs_public_keys_vargen_dev(vc.FORMAT_CODE[fmt], _ptr(cols[0]), _ptr(cols[1]), ng, n, _ptr(PK), _ptr(G_out), _ptr(st), _stream())
    assert rc == 0, lib().jjs_last_error()
    torch.cuda.synchronize()
    return PK.cpu().numpy(), G_out.cpu().numpy(), st.cpu().numpy()


def _odd(a):
    """A copy at an odd address: the host forms ask for no alignment."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    raw = np.empty(a.nbytes + 17, np.uint8)
    at = 1 + (-raw.ctypes.data) % 16
    out = raw[at:at + a.nbytes].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 2 == 1
    return out


def _h(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def sign_host(fmt, sk, Gen, rnd, m, odd=True):
    wrap = _odd if odd else np.ascontiguousarray
    n, ng = len(sk), len(Gen)
    ins = [wrap(x) for x in (sk, Gen, rnd, m)]
    u, R, PK, G_out, st = (wrap(np.full(s, FILL, np.uint8)) for s in ((n, 32), (n, 64), (n, 64), (ng, 64), (n,)))
    rc = lib().jjs_sign_vargen_pt(vc.FORMAT_CODE[fmt], _h(ins[0]), _h(ins[1]), ng, _h(ins[2]), _h(ins[3]), n, _h(u), _h(R), _h(PK), _h(G_out), _h(st))
    assert rc == 0, lib().jjs_last_error()
    return u, R, PK, G_out, st


def derive_host(fmt, sk, Gen):
    n, ng = len(sk), len(Gen)
    ins = [_odd(sk), _odd(Gen)]
    PK, G_out, st = (_odd(np.full(s, FILL, np.uint8)) for s in ((n, 64), (ng, 64), (n,)))
    rc = lib().jjs_public_keys_vargen(vc.FORMAT_CODE[fmt], _h(ins[0]), _h(ins[1]), ng, n, _h(PK), _h(G_out), _h(st))
    assert rc == 0, lib().jjs_last_error()
    return PK, G_out, st


# ---- (a) the reference's own bytes ---------------------------------------------------------------------------------------------
def test_the_references_own_bytes_in_wire_format(eng, reference_kat):
    k = vc.kat(reference_kat)
    sk = np.frombuffer(k["secret"][:32], np.uint8).reshape(1, 32)
    gen_w = np.frombuffer(k["secret"][32:], np.uint8).reshape(1, 32)
    PK, G_out, st = derive_host("wire", sk, gen_w)
    assert st.tolist() == [0] and o.compress(to_pt(PK[0])) + o.compress(to_pt(G_out[0])) == k["public"]
    u, R, PK2, G2, st = sign_host("wire", sk, gen_w, k["rnd"].reshape(1, 32), k["m"].reshape(1, 32))
    assert st.tolist() == [0] and (PK2 == PK).all() and (G2 == G_out).all()
    assert u[0].tobytes() + o.compress(to_pt(R[0])) == k["signature"]
    # ... and through the mirror's type, which holds the 64 bytes as the reference serialises them
    import jubjub_schnorr_amd as jjs
    key = jjs.SecretKeyVarGen.from_bytes(k["secret"])
    pk = key.public_key()
    sig = key.sign(k["rnd"].tobytes(), k["m"].tobytes())
    assert o.compress(to_pt(np.frombuffer(pk.pk, np.uint8))) + o.compress(to_pt(np.frombuffer(pk.generator, np.uint8))) == k["public"]
    assert sig.u + o.compress(to_pt(np.frombuffer(sig.R, np.uint8))) == k["signature"]
    pk.verify(sig, k["m"].tobytes())
    affine = jjs.SecretKeyVarGen.new(key.sk, pk.generator)
    assert affine.to_bytes() == k["secret"] and affine.sign(k["rnd"].tobytes(), k["m"].tobytes()) == sig
    with pytest.raises(jjs.Malformed):
        jjs.SecretKeyVarGen.from_bytes(k["secret"][:32] + b"\xff" * 32).public_key()
    with pytest.raises(jjs.Malformed):
        jjs.SecretKeyVarGen.new(key.sk, pk.generator).sign(b"\xff" * 32, k["m"].tobytes())


# ---- (b), (d) every case, one call per format ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", vc.FORMATS)
def test_every_case_in_one_call(eng, fmt):
    c = vc.call(fmt)
    assert c.n == 64 and all(c.status[i] == 3 for i in vc.FIRST_PLACES)
    got = sign_dev(fmt, c.sk, c.Gen, c.rnd, c.m)
    vc.check(got, c, (fmt, "_dev"))
    vc.check(sign_host(fmt, c.sk, c.Gen, c.rnd, c.m), c, (fmt, "host, unaligned"))
    vc.check(sign_host(fmt, c.sk, c.Gen, c.rnd, c.m, odd=False), c, (fmt, "host"))
    u, R, PK, G_out, st = sign_dev(fmt, c.sk, c.Gen, c.rnd, c.m, want_pk=False, want_gen=False)
    assert PK is None and G_out is None and (u == c.u).all() and (R == c.R).all() and st.tolist() == c.status.tolist()
    # the derivation: a row with a bad rnd or m is a good row to it
    for PK, G_out, st in (derive_dev(fmt, c.sk, c.Gen), derive_host(fmt, c.sk, c.Gen)):
        for i in range(c.n):
            if c.status[i] == 0:
                assert st[i] == 0 and (PK[i] == c.PK[i]).all() and (G_out[i] == c.Gen_out[i]).all(), (fmt, c.labels[i])
            elif "rnd=r" in c.labels[i] or "m=q" in c.labels[i]:
                assert st[i] == 0 and (PK[i] != FILL).any() and (G_out[i] != FILL).any(), (fmt, c.labels[i])
            else:
                assert st[i] == 3 and not PK[i].any() and not G_out[i].any(), (fmt, c.labels[i])
    # (d) what PublicKeyVarGen::verify says about the signatures: exactly the oracle's status
    good = np.nonzero(c.status == 0)[0]
    u, R, PK, G_out, _ = got
    st, _ = eng.verify("vargen", u[good], R[good], PK[good], G_out[good], c.m[good])
    assert st.tolist() == c.verify[good].tolist()
    assert set(st.tolist()) == {0, 1}, "prime-order generators verify, the identity, small-order and torsion generators are InvalidPoint"


# ---- (c) against the signer that takes the generator as a scalar ------------------------------------------------------------------
def _random_scalars(rng, n):
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0D                          # < 0x0E00.. < r < q
    return a


def _scalar_signer(eng, n, seed):
    """sk, gen_scalar, rnd, m and what jjs_sign_vargen_dev gives for them (torch device tensors)."""
    rng = np.random.default_rng(seed)
    cols = [dev(_random_scalars(rng, n)) for _ in range(4)]
    return cols, eng.sign("vargen", cols[0], cols[2], cols[3], gen_scalar=cols[1])


def _formats_of(eng, Gen):
    """The affine generator column (device tensor) in the three formats."""
    return {"affine": Gen, "ext": dev(to_extended(Gen.cpu().numpy(), np.random.default_rng(5))), "wire": eng.compress(Gen)}


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_equal_to_the_scalar_signer(eng, n):
    import torch
    (sk, _, rnd, m), want = _scalar_signer(eng, n, 1800 + n)
    for fmt, Gen in _formats_of(eng, want[3]).items():
        got = eng.sign_vargen_pt(sk, Gen, rnd, m, fmt=fmt)
        torch.cuda.synchronize()
        for name, a, b in zip(("u", "R", "PK", "Gen"), got, want):
            assert torch.equal(a, b), (n, fmt, name)
        assert not got[4].any(), (n, fmt, "status")
        PK, G_out, st = eng.public_keys_vargen(sk, Gen, fmt=fmt)
        assert torch.equal(PK, want[2]) and torch.equal(G_out, want[3]) and not st.any(), (n, fmt, "derivation")
    st, _ = eng.verify("vargen", want[0], want[1], want[2], want[3], m)
    assert not st.any()


# ---- (e) the grid-stride loop's second trip --------------------------------------------------------------------------------------
def test_one_item_more_than_the_resident_lanes(eng):
    import torch
    resident = eng.sign_limits()["resident_lanes"]
    assert 0 < resident <= 1 << 20
    n = resident + 1
    (sk, _, rnd, m), want = _scalar_signer(eng, n, 1900)
    got = eng.sign_vargen_pt(sk, want[3], rnd, m)
    torch.cuda.synchronize()
    for name, a, b in zip(("u", "R", "PK", "Gen"), got, want):
        assert torch.equal(a, b), name
    assert not got[4].any()
    rows = [0, resident - 1, resident, n - 1]
    host = [x[rows].cpu().numpy() for x in (sk, want[3], rnd, m, got[0], got[1], got[2])]
    for j, i in enumerate(rows):
        p = to_pt(host[1][j])
        wu, wR, wPK = vc.oracle_rows(host[0], p, host[2], host[3], [j])[j]
        assert (host[4][j] == wu).all() and (host[5][j] == wR).all() and (host[6][j] == wPK).all(), i


# ---- (f) one generator for the call ----------------------------------------------------------------------------------------------
def _shared_sizes(eng):
    t = eng.sign_limits()["shared_generator_from"]
    return (1, 64, 257) + ((t - 1, t, t + 1) if t is not None else ())


@pytest.mark.parametrize("which", vc.SHARED_GENERATORS + ("unusable",))
def test_one_generator_for_the_call(eng, which):
    for n in _shared_sizes(eng):
        for fmt in vc.FORMATS if n <= 64 else ("affine",):
            sk, Gen, rnd, m, p = vc.shared_call(which, n, fmt)
            one = sign_dev(fmt, sk, Gen, rnd, m)
            tiled = sign_dev(fmt, sk, np.tile(Gen, (n, 1)), rnd, m)
            for k in (0, 1, 2, 4):
                assert (one[k] == tiled[k]).all(), (which, n, fmt, k)
            assert one[3].shape == (1, 64) and (tiled[3] == one[3][0]).all()
            PK, G_out, st = derive_dev(fmt, sk, Gen)
            assert (PK == one[2]).all() and (G_out == one[3]).all() and (st == one[4]).all(), (which, n, fmt, "derivation")
            if which == "unusable":
                assert one[4].tolist() == [3] * n and not any(x.any() for x in one[:4]), (n, fmt)
            else:
                assert not one[4].any() and to_pt(one[3][0]) == p
                for i, (wu, wR, wPK) in vc.oracle_rows(sk, p, rnd, m, sorted({0, min(1, n - 1), n - 1})).items():
                    assert (one[0][i] == wu).all() and (one[1][i] == wR).all() and (one[2][i] == wPK).all(), (which, n, fmt, i)
    host = sign_host("affine", *vc.shared_call(which, 64)[:4])
    again = sign_dev("affine", *vc.shared_call(which, 64)[:4])
    for a, b in zip(host, again):
        assert (a == b).all(), (which, "the host form")


# ---- (g) return codes -------------------------------------------------------------------------------------------------------------
def test_return_codes_and_nothing_written(eng):
    import torch
    c = vc.call("affine")
    cols = [dev(x) for x in (c.sk, c.Gen, c.rnd, c.m)]
    outs = [_filled(64, 32), _filled(64, 64), _filled(64, 64), _filled(64, 64), _filled(64)]

    def call(fmt=0, ng=64, n=64, cols=cols, outs=outs):
        return lib().jjs_sign_vargen_pt_dev(fmt, _ptr(cols[0]), _ptr(cols[1]), ng, _ptr(cols[2]), _ptr(cols[3]), n, *[_ptr(x) for x in outs], _stream())

    def derive(fmt=0, ng=64, n=64, sk=cols[0], gen=cols[1], PK=outs[2], st=outs[4]):
        return lib().jjs_public_keys_vargen_dev(fmt, _ptr(sk), _ptr(gen), ng, n, _ptr(PK), _ptr(outs[3]), _ptr(st), _stream())

    assert call(n=0, ng=0) == 0 and call(n=0, ng=5) == 0 and derive(n=0, ng=0) == 0, "n == 0 returns 0"
    assert call(fmt=3) == -1 and call(fmt=-1) == -1 and derive(fmt=3) == -1, "a bad format"
    assert call(ng=2) == -1 and call(ng=0) == -1 and call(ng=63) == -1 and derive(ng=65) == -1, "a bad n_gen"
    for k in range(4):
        assert call(cols=[None if j == k else x for j, x in enumerate(cols)]) == -1, ("a NULL input", k)
    for k in (0, 1, 4):
        assert call(outs=[None if j == k else x for j, x in enumerate(outs)]) == -1, ("a NULL required output", k)
    assert derive(PK=None) == -1 and derive(st=None) == -1 and derive(sk=None) == -1 and derive(gen=None) == -1
    for k in range(4):
        assert call(cols=[x.view(-1)[8:] if j == k else x for j, x in enumerate(cols)], n=32, ng=32) == -1, ("a misaligned input", k)
    for k in range(4):
        assert call(outs=[x.view(-1)[8:] if j == k else x for j, x in enumerate(outs)], n=32, ng=32) == -1, ("a misaligned output", k)
    assert b"misaligned" in lib().jjs_last_error()
    torch.cuda.synchronize()
    assert all(bool((x == FILL).all()) for x in outs), "a refused call writes nothing"
    h = [np.ascontiguousarray(x) for x in (c.sk, c.Gen, c.rnd, c.m)]
    ho = [np.full(s, FILL, np.uint8) for s in ((64, 32), (64, 64), (64,))]
    host = lambda fmt, ng, n, sk=h[0]: lib().jjs_sign_vargen_pt(fmt, _h(sk), _h(h[1]), ng, _h(h[2]), _h(h[3]), n, _h(ho[0]), _h(ho[1]), None, None, _h(ho[2]))  # noqa: E731
    assert host(0, 0, 0) == 0 and host(5, 64, 64) == -1 and host(0, 7, 64) == -1 and host(0, 64, 64, None) == -1
    assert lib().jjs_public_keys_vargen(0, _h(h[0]), _h(h[1]), 64, 64, None, None, _h(ho[2])) == -1
    assert all((x == FILL).all() for x in ho)
    # status needs no alignment; PK_out and Gen_out may be NULL
    st = _filled(65)
    assert call(outs=[outs[0], outs[1], None, None, st[1:]]) == 0
    torch.cuda.synchronize()
    assert st[1:].cpu().numpy().tolist() == c.status.tolist() and int(st[0]) == FILL
    limits = (ctypes.c_uint64 * 2)()
    assert lib().jjs_debug_sign_limits(limits) == 0 and lib().jjs_debug_sign_limits(None) == -1
    assert limits[0] % 256 == 0 and limits[0] > 0


def test_no_allocation_at_a_shape_the_engine_has_seen_and_trim(eng):
    sk, Gen, rnd, m, _ = vc.shared_call("5*G", 257, "ext")
    sign_host("ext", sk, Gen, rnd, m)
    before = eng.memory_stats()
    one = sign_host("ext", sk, Gen, rnd, m)
    assert eng.memory_stats() == before, "the second call of a shape allocates nothing"
    eng.trim()
    two = sign_host("ext", sk, Gen, rnd, m)
    for a, b in zip(one, two):
        assert (a == b).all()


def test_shared_generator_route_forced():
    p = subprocess.run([sys.executable, os.path.join(HERE, "sign_vargen_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]

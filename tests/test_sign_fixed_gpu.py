"""jjs_sign_fixed(_dev) and jjs_public_keys_fixed(_dev) on the device, through the C ABI with every output prefilled with 0xA5.
Expected values: the reference's own bytes, the oracle's (sign_fixed_cases.py), and jjs_sign_single_dev / jjs_sign_double_dev, the
old signers, which must give the same bytes for in-range inputs.  Every comparison is byte for byte.  Then sign_fixed_child.py
forces both routes of a call with one key (profiling build)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import jjs_oracle as o
import sign_fixed_cases as fc
from helpers import fe_bytes, to_int, to_pt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xA5
SCHEMES = (False, True)
NAME = {False: "single", True: "double"}


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


def _shapes(double, n, n_sk):
    w = fc.widths(double)
    return {k: ((n_sk if k in ("PK", "PKp", "pk_w") else n), w[k]) for k in fc.outputs_of(double)}


def sign_dev(double, sk, rnd, m, skip=()):
    """jjs_sign_fixed_dev with prefilled outputs -> {name: numpy, "status": numpy} (None for a skipped output)."""
    import torch
    n, nk = len(rnd), len(sk)
    cols = [dev(x) for x in (sk, rnd, m)]
    shapes = _shapes(double, n, nk)
    outs = {k: (_filled(*shapes[k]) if k in shapes and k not in skip else None) for k in fc.OUTPUTS}
    st = _filled(n)
    rc = lib().jjs_sign_fixed_dev(int(double), _ptr(cols[0]), nk, _ptr(cols[1]), _ptr(cols[2]), n, *[_ptr(outs[k]) for k in fc.OUTPUTS], _ptr(st), _stream())
    assert rc == 0, lib().jjs_last_error()
    torch.cuda.synchronize()
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in outs.items()}
    got["status"] = st.cpu().numpy()
    for k, v in got.items():
        if v is not None:
            assert not (v.reshape(len(v), -1) == FILL).all(1).any(), (k, "an output row was not written")
    return got


def derive_dev(double, sk, skip=()):
    import torch
    n = len(sk)
    shapes = _shapes(double, n, n)
    outs = {k: (_filled(*shapes[k]) if k in shapes and k not in skip else None) for k in ("PK", "PKp", "pk_w")}
    st = _filled(n)
    t = dev(sk)
    rc = lib().jjs_public_keys_fixed_dev(int(double), _ptr(t), n, _ptr(outs["PK"]), _ptr(outs["PKp"]), _ptr(outs["pk_w"]), _ptr(st), _stream())
    assert rc == 0, lib().jjs_last_error()
    torch.cuda.synchronize()
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in outs.items()}
    got["status"] = st.cpu().numpy()
    return got


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


def sign_host(double, sk, rnd, m, odd=True, skip=()):
    wrap = _odd if odd else np.ascontiguousarray
    n, nk = len(rnd), len(sk)
    ins = [wrap(x) for x in (sk, rnd, m)]
    shapes = _shapes(double, n, nk)
    outs = {k: (wrap(np.full(shapes[k], FILL, np.uint8)) if k in shapes and k not in skip else None) for k in fc.OUTPUTS}
    st = wrap(np.full(n, FILL, np.uint8))
    rc = lib().jjs_sign_fixed(int(double), _h(ins[0]), nk, _h(ins[1]), _h(ins[2]), n, *[_h(outs[k]) for k in fc.OUTPUTS], _h(st))
    assert rc == 0, lib().jjs_last_error()
    outs["status"] = st
    return outs


def derive_host(double, sk, skip=()):
    n = len(sk)
    shapes = _shapes(double, n, n)
    outs = {k: (_odd(np.full(shapes[k], FILL, np.uint8)) if k in shapes and k not in skip else None) for k in ("PK", "PKp", "pk_w")}
    st = _odd(np.full(n, FILL, np.uint8))
    rc = lib().jjs_public_keys_fixed(int(double), _h(_odd(sk)), n, _h(outs["PK"]), _h(outs["PKp"]), _h(outs["pk_w"]), _h(st))
    assert rc == 0, lib().jjs_last_error()
    outs["status"] = st
    return outs


def _same(a, b, label, names=None):
    for k in names or [k for k in a if a[k] is not None]:
        assert (a[k] == b[k]).all(), (label, k)


# ---- 1. the reference's own bytes -------------------------------------------------------------------------------------------------
def test_the_references_own_bytes(eng, reference_kat):
    import jubjub_schnorr_amd as jjs
    k = fc.kat(reference_kat)
    sk, m = k["sk"].reshape(1, 32), k["m"].reshape(1, 32)
    s = sign_host(False, sk, k["rnd"].reshape(1, 32), m, skip=("u", "R", "PK"))
    assert s["status"].tolist() == [0] and s["sig_w"][0].tobytes() == k["signature"] and s["pk_w"][0].tobytes() == k["public"]
    d = sign_host(True, sk, k["rnd_double"].reshape(1, 32), m, skip=("u", "R", "Rp", "PK", "PKp"))
    assert d["status"].tolist() == [0] and d["sig_w"][0].tobytes() == k["signature_double"] and d["pk_w"][0].tobytes() == k["public_double"]
    assert derive_host(False, sk)["pk_w"][0].tobytes() == k["public"] and derive_host(True, sk)["pk_w"][0].tobytes() == k["public_double"]
    pairs = derive_host(False, np.stack([x for x, _ in k["pairs"]]))
    assert pairs["status"].tolist() == [0, 0, 0] and [r.tobytes() for r in pairs["pk_w"]] == [p for _, p in k["pairs"]]
    # ... and through the mirror's type
    key = jjs.SecretKey.from_bytes(k["secret"])
    pk, pkd = key.public_key(), key.public_key_double()
    comp = lambda b: o.compress(to_pt(np.frombuffer(b, np.uint8)))  # noqa: E731
    assert comp(pk.point) == k["public"] and comp(pkd.pk) + comp(pkd.pk_prime) == k["public_double"]
    sig = key.sign(k["rnd"].tobytes(), k["m"].tobytes())
    assert sig.u + comp(sig.R) == k["signature"]
    pk.verify(sig, k["m"].tobytes())
    sd = key.sign_double(k["rnd_double"].tobytes(), k["m"].tobytes())
    assert sd.u + comp(sd.R) + comp(sd.R_prime) == k["signature_double"]
    pkd.verify(sd, k["m"].tobytes())
    # the batches: one call, a key per item or one key for the call
    other = jjs.SecretKey.from_bytes(bytes([5]) + bytes(31))
    batch = jjs.SecretKey.sign_batch([(key, k["rnd"].tobytes(), k["m"].tobytes()), (other, k["rnd"].tobytes(), k["m"].tobytes()),
                                      (key, k["rnd"].tobytes(), k["m"].tobytes())])
    assert batch[0] == sig and batch[2] == sig and batch[1] != sig
    other.public_key().verify(batch[1], k["m"].tobytes())
    assert jjs.SecretKey.sign_double_batch([(key, k["rnd_double"].tobytes(), k["m"].tobytes())] * 3) == [sd] * 3
    with pytest.raises(jjs.Malformed):
        key.sign(b"\xff" * 32, k["m"].tobytes())
    with pytest.raises(jjs.Malformed):
        jjs.SecretKey(o.le32(o.R_ORDER)).public_key()           # the constructor does not test the range: the engine does
    with pytest.raises(jjs.Malformed):
        jjs.SecretKey.sign_batch([(key, k["rnd"].tobytes(), k["m"].tobytes()), (key, k["rnd"].tobytes(), b"\xff" * 32)])


# ---- 2. every case in one call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", SCHEMES)
def test_every_case_in_one_call(eng, double):
    c = fc.call(double)
    assert c.n == 64 and all(c.status[i] == 3 for i in fc.PLACES)
    got = sign_dev(double, c.sk, c.rnd, c.m)
    fc.check(got, c, (double, "_dev"))
    fc.check(sign_host(double, c.sk, c.rnd, c.m), c, (double, "host, unaligned"))
    fc.check(sign_host(double, c.sk, c.rnd, c.m, odd=False), c, (double, "host"))
    for name in fc.outputs_of(double):
        fc.check(sign_dev(double, c.sk, c.rnd, c.m, skip=(name,)), c, (double, "without", name), skip=(name,))
    fc.check(sign_host(double, c.sk, c.rnd, c.m, skip=("u", "R", "Rp", "PK", "PKp")), c, (double, "host, wire alone"), skip=("u", "R", "Rp", "PK", "PKp"))
    # the derivation: a row with a bad rnd or m is a good row to it
    for d in (derive_dev(double, c.sk), derive_host(double, c.sk), derive_dev(double, c.sk, skip=("PK", "PKp"))):
        for i in range(c.n):
            sk = to_int(c.sk[i])
            want = fc.key_rows(double, sk) if sk < o.R_ORDER else {k: 0 for k in fc.key_rows(double, 0)}
            assert d["status"][i] == (0 if sk < o.R_ORDER else 3), c.labels[i]
            for k, w in want.items():
                assert d[k] is None or (d[k][i] == w).all(), (k, c.labels[i])
    # what PublicKey::verify / PublicKeyDouble::verify say about the signatures: exactly the oracle's status
    good = np.nonzero(c.status == 0)[0]
    cols = [got[k][good] for k in (("u", "R", "Rp", "PK", "PKp") if double else ("u", "R", "PK"))] + [c.m[good]]
    st, _ = eng.verify(NAME[double], *cols)
    assert st.tolist() == c.verify[good].tolist()
    assert sorted(set(st.tolist())) == [0, 1], "sk = 0 signs, and its key, the identity, is InvalidPoint"


def test_scheme_foreign_outputs_are_refused(eng):
    c = fc.call(False)
    cols = [dev(x) for x in (c.sk, c.rnd, c.m)]
    u, R, X, st = _filled(64, 32), _filled(64, 64), _filled(64, 64), _filled(64)
    L = lib()
    assert L.jjs_sign_fixed_dev(0, _ptr(cols[0]), 64, _ptr(cols[1]), _ptr(cols[2]), 64, _ptr(u), _ptr(R), _ptr(X), None, None, None, None, _ptr(st), _stream()) == -1
    assert L.jjs_sign_fixed_dev(0, _ptr(cols[0]), 64, _ptr(cols[1]), _ptr(cols[2]), 64, _ptr(u), _ptr(R), None, None, _ptr(X), None, None, _ptr(st), _stream()) == -1
    assert L.jjs_public_keys_fixed_dev(0, _ptr(cols[0]), 64, _ptr(R), _ptr(X), None, _ptr(st), _stream()) == -1
    assert L.jjs_sign_fixed_dev(1, _ptr(cols[0]), 64, _ptr(cols[1]), _ptr(cols[2]), 64, _ptr(u), _ptr(R), _ptr(X), None, None, None, None, _ptr(st), _stream()) == 0
    import torch
    torch.cuda.synchronize()


# ---- 3. equal to the old signer -----------------------------------------------------------------------------------------------------
def _random_scalars(rng, n):
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0D                          # < 0x0E00.. < r < q
    return a


def _old_signer(eng, double, n, seed):
    """sk, rnd, m and what jjs_sign_single_dev / jjs_sign_double_dev give for them (torch device tensors)."""
    rng = np.random.default_rng(seed)
    cols = [dev(_random_scalars(rng, n)) for _ in range(3)]
    return cols, eng.sign(NAME[double], *cols)


def _equal_to_old(eng, double, cols, want, got, label):
    import torch
    names = ("u", "R", "Rp", "PK", "PKp") if double else ("u", "R", "PK")
    for name, a, b in zip(names, got, want):
        assert torch.equal(a, b), (label, name)
    sig_w, pk_w, st = got[len(names):]
    assert not st.any(), (label, "status")
    pts = [eng.compress(x) for x in want[1:]]
    assert torch.equal(sig_w, torch.cat([want[0]] + pts[:2 if double else 1], 1)), (label, "sig_w")
    assert torch.equal(pk_w, torch.cat(pts[2 if double else 1:], 1)), (label, "pk_w")


@pytest.mark.parametrize("double", SCHEMES)
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257))
def test_equal_to_the_old_signer(eng, double, n):
    import torch
    cols, want = _old_signer(eng, double, n, 2000 + n)
    got = eng.sign_fixed(NAME[double], *cols, wire=True)
    torch.cuda.synchronize()
    _equal_to_old(eng, double, cols, want, got, (double, n))
    d = eng.public_keys_fixed(NAME[double], cols[0], wire=True)
    k = 2 if double else 1
    for a, b in zip(d[:k], want[-k:]):
        assert torch.equal(a, b), (double, n, "derivation")
    assert torch.equal(d[k], got[-2]) and not d[-1].any()


# ---- 4. one key for the call ----------------------------------------------------------------------------------------------------------
def _keyed_sizes(eng):
    t = eng.sign_fixed_limits()["keyed_from"]
    return (1, 2, 64, 257) + ((t - 1, t, t + 1) if t is not None and t <= 1 << 16 else ())


@pytest.mark.parametrize("double", SCHEMES)
@pytest.mark.parametrize("which", fc.KEYED_KEYS)
def test_one_key_for_the_call(eng, double, which):
    names = fc.outputs_of(double)
    key_names = [k for k in names if k in ("PK", "PKp", "pk_w")]
    for n in _keyed_sizes(eng):
        sk, rnd, m = fc.keyed_call(double, which, n)
        one = sign_dev(double, sk, rnd, m)
        tiled = sign_dev(double, np.tile(sk, (n, 1)), rnd, m)
        _same(one, tiled, (which, n, "against the key tiled"), [k for k in names if k not in key_names] + ["status"])
        assert all(one[k].shape[0] == 1 for k in key_names)
        _same(one, sign_host(double, sk, rnd, m), (which, n, "the host form"))
        if which == "unusable":
            assert one["status"].tolist() == [3] * n and not any(one[k].any() for k in names), (which, n)
            continue
        bad_first = n > 2                      # keyed_call: row 0 has rnd = r
        assert one["status"].tolist() == ([3] if bad_first else [0]) + [0] * (n - 1)
        for k, w in fc.key_rows(double, fc.keyed_key(which)).items():
            assert (one[k][0] == w).all() and (tiled[k][n - 1] == w).all(), (which, n, k)
        rows = [i for i in sorted({0, 1, n - 1}) if i < n and not (bad_first and i == 0)]
        for i, w in fc.oracle_rows(double, sk, rnd, m, rows).items():
            for k in names:
                if k not in key_names:
                    assert (one[k][i] == w[k]).all(), (which, n, k, i)


# ---- 5. the grid-stride loop's second trip ----------------------------------------------------------------------------------------------
def test_one_item_more_than_the_resident_lanes(eng):
    import torch
    resident = eng.sign_fixed_limits()["resident_lanes"]
    assert 0 < resident <= 1 << 20 and resident % 256 == 0
    n = resident + 1
    cols, want = _old_signer(eng, False, n, 2100)
    got = eng.sign_fixed("single", *cols, wire=True)
    torch.cuda.synchronize()
    _equal_to_old(eng, False, cols, want, got, "a key per item")
    rows = [0, resident - 1, resident, n - 1]
    host = [x[rows].cpu().numpy() for x in cols]
    for j, w in fc.oracle_rows(False, *host, range(4)).items():
        assert (got[0][rows[j]].cpu().numpy() == w["u"]).all() and (got[1][rows[j]].cpu().numpy() == w["R"]).all(), rows[j]
        assert (got[3][rows[j]].cpu().numpy() == w["sig_w"]).all(), rows[j]
    # one key for the call: the old signer on the key tiled
    key = cols[0][:1].contiguous()
    tiled = key.expand(n, 32).contiguous()
    want = eng.sign("single", tiled, cols[1], cols[2])
    got = eng.sign_fixed("single", key, cols[1], cols[2], wire=True)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not got[-1].any()
    assert got[2].shape == (1, 64) and torch.equal(got[2], want[2][:1]) and torch.equal(got[4], eng.compress(want[2][:1]))
    host = [key.cpu().numpy()] + [x[rows].cpu().numpy() for x in cols[1:]]
    for j, w in fc.oracle_rows(False, *host, range(4)).items():
        assert (got[3][rows[j]].cpu().numpy() == w["sig_w"]).all(), rows[j]


def test_the_keyed_route_by_size(eng):
    """The product build takes the keyed route by size alone: at the reported threshold, one key for the call against the old
    signers on the key tiled, both schemes."""
    import torch
    t = eng.sign_fixed_limits()["keyed_from"]
    if t is None or t > 1 << 20:
        return                                 # no call of a testable size takes it: sign_fixed_child.py forces it
    rng = np.random.default_rng(2200)
    key, rnd, m = dev(_random_scalars(rng, 1)), dev(_random_scalars(rng, t)), dev(_random_scalars(rng, t))
    tiled = key.expand(t, 32).contiguous()
    for double in SCHEMES:
        want = eng.sign(NAME[double], tiled, rnd, m)
        got = eng.sign_fixed(NAME[double], key, rnd, m)
        torch.cuda.synchronize()
        k = 3 if double else 2
        assert all(torch.equal(a, b) for a, b in zip(got[:k], want[:k])) and not got[-1].any(), double
        assert all(a.shape == (1, 64) and torch.equal(a, b[:1]) for a, b in zip(got[k:-1], want[k:])), double


# ---- 6. return codes -------------------------------------------------------------------------------------------------------------------
def test_return_codes_and_nothing_written(eng):
    import torch
    c = fc.call(True)
    cols = [dev(x) for x in (c.sk, c.rnd, c.m)]
    outs = [_filled(64, 32), _filled(64, 64), _filled(64, 64), _filled(64, 64), _filled(64, 64), _filled(64, 96), _filled(64, 64), _filled(64)]

    def call(scheme=1, nk=64, n=64, cols=cols, outs=outs):
        return lib().jjs_sign_fixed_dev(scheme, _ptr(cols[0]), nk, _ptr(cols[1]), _ptr(cols[2]), n, *[_ptr(x) for x in outs], _stream())

    def derive(scheme=1, n=64, sk=cols[0], PK=outs[3], PKp=outs[4], pk_w=outs[6], st=outs[7]):
        return lib().jjs_public_keys_fixed_dev(scheme, _ptr(sk), n, _ptr(PK), _ptr(PKp), _ptr(pk_w), _ptr(st), _stream())

    assert call(n=0, nk=0) == 0 and call(n=0, nk=5) == 0 and derive(n=0) == 0, "n == 0 returns 0"
    assert call(scheme=2) == -1 and call(scheme=3) == -1 and call(scheme=-1) == -1 and derive(scheme=2) == -1, "a bad scheme"
    assert call(nk=2) == -1 and call(nk=0) == -1 and call(nk=63) == -1 and call(nk=65) == -1, "a bad n_sk"
    for k in range(3):
        assert call(cols=[None if j == k else x for j, x in enumerate(cols)]) == -1, ("a NULL input", k)
    assert call(outs=outs[:7] + [None]) == -1 and derive(st=None) == -1 and derive(sk=None) == -1, "status is required"
    assert call(outs=[None, None, None, outs[3], outs[4], None, outs[6], outs[7]]) == -1, "no signature output"
    assert derive(PK=None, PKp=None, pk_w=None) == -1, "no key output"
    for k in range(3):
        assert call(cols=[x.view(-1)[8:] if j == k else x for j, x in enumerate(cols)], n=32, nk=32) == -1, ("a misaligned input", k)
    for k in range(7):
        assert call(outs=[x.view(-1)[8:] if j == k else x for j, x in enumerate(outs)], n=32, nk=32) == -1, ("a misaligned output", k)
    assert b"misaligned" in lib().jjs_last_error()
    assert derive(PK=outs[3].view(-1)[8:], n=32) == -1
    torch.cuda.synchronize()
    assert all(bool((x == FILL).all()) for x in outs), "a refused call writes nothing"
    h = [np.ascontiguousarray(x) for x in (c.sk, c.rnd, c.m)]
    ho = [np.full(s, FILL, np.uint8) for s in ((64, 32), (64, 64), (64,))]
    host = lambda scheme, nk, n, sk=h[0], u=ho[0]: lib().jjs_sign_fixed(scheme, _h(sk), nk, _h(h[1]), _h(h[2]), n, _h(u), None, None, None, None, None, None, _h(ho[2]))  # noqa: E731
    assert host(1, 0, 0) == 0 and host(2, 64, 64) == -1 and host(1, 7, 64) == -1 and host(1, 64, 64, None) == -1 and host(1, 64, 64, h[0], None) == -1
    assert lib().jjs_sign_fixed(0, _h(h[0]), 64, _h(h[1]), _h(h[2]), 64, _h(ho[0]), None, _h(ho[1]), None, None, None, None, _h(ho[2])) == -1, "R' in the single scheme"
    assert lib().jjs_public_keys_fixed(1, _h(h[0]), 64, None, None, None, _h(ho[2])) == -1
    assert all((x == FILL).all() for x in ho)
    # status needs no alignment; one output is enough
    st = _filled(65)
    assert call(outs=[outs[0], None, None, None, None, None, None, st[1:]]) == 0
    torch.cuda.synchronize()
    assert st[1:].cpu().numpy().tolist() == c.status.tolist() and int(st[0]) == FILL and (outs[0].cpu().numpy() == c.want["u"]).all()
    limits = (ctypes.c_uint64 * 2)()
    assert lib().jjs_debug_sign_fixed_limits(limits) == 0 and lib().jjs_debug_sign_fixed_limits(None) == -1
    assert limits[0] % 256 == 0 and limits[0] > 0 and limits[1] >= 2


# ---- 7. allocation ------------------------------------------------------------------------------------------------------------------------
def test_no_allocation_at_a_shape_the_engine_has_seen_and_trim(eng):
    import torch
    for double in SCHEMES:
        sk, rnd, m = fc.keyed_call(double, "random", 257)
        sign_host(double, sk, rnd, m)
        sign_dev(double, sk, rnd, m)
        derive_host(double, np.tile(sk, (257, 1)))
        before = eng.memory_stats()
        one = sign_host(double, sk, rnd, m)
        dev_one = sign_dev(double, sk, rnd, m)
        derive_host(double, np.tile(sk, (257, 1)))
        torch.cuda.synchronize()
        assert eng.memory_stats() == before, "the second call of a shape allocates nothing"
        eng.trim()
        _same(one, sign_host(double, sk, rnd, m), "after jjs_trim")
        _same(dev_one, one, "the host form and the _dev form")


# ---- 8. both routes forced --------------------------------------------------------------------------------------------------------------
def test_both_routes_forced():
    p = subprocess.run([sys.executable, os.path.join(HERE, "sign_fixed_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]

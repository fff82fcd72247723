"""The CPU build of csrc/msm.h and csrc/batch_verdict.h (the batch verdict of jjs_verify_all_*) against the oracle: the
bucket MSM against o.mul / o.add, the ChaCha20 block against RFC 8439, and the whole verdict against all(status == 0) of
the oracle for the three schemes.  No GPU."""
import json
import os

import numpy as np
import pytest

import jjs_oracle as o
import verdict_hostlib as vh
from helpers import ARG_ORDER, edge_cases, fe_bytes, make_batch, oracle_verify, pt_bytes, to_pt, torsion_generator, torsion_grid

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMES = ["single", "double", "vargen"]


def test_chacha20_block_rfc8439_vector():
    v = json.load(open(os.path.join(HERE, "golden", "chacha20_rfc8439.json")))
    out = vh.chacha20_block(bytes.fromhex(v["key"]), v["counter"], bytes.fromhex(v["nonce"]))
    assert out.hex() == v["block"]


def _points(rng, n):
    return [o.mul(o.G, int(rng.integers(1, 1 << 62)) * 7919 + 1) for _ in range(n)]


def _msm_oracle(pts, ks, neg):
    acc = o.IDENTITY
    for p, k, s in zip(pts, ks, neg):
        q = o.mul(p, k)
        acc = o.add(acc, o.neg(q) if s else q)
    return acc


@pytest.mark.parametrize("n", [1, 2, 7, 100, 1000])
def test_msm_matches_oracle(n):
    rng = np.random.default_rng(n)
    pts = _points(rng, min(n, 40))
    pts = [pts[i % len(pts)] for i in range(n)]
    special = [0, 1, o.R_ORDER - 1, (1 << 128) - 1, (1 << 252) - 1 if (1 << 252) - 1 < o.R_ORDER else o.R_ORDER - 2]
    ks = [special[i] if i < len(special) else int.from_bytes(rng.bytes(32), "little") % o.R_ORDER for i in range(n)]
    neg = [int(rng.integers(0, 2)) for _ in range(n)]
    want = _msm_oracle(pts, ks, neg)
    scal = np.stack([fe_bytes(k) for k in ks])
    parr = np.stack([pt_bytes(p) for p in pts])
    for c in ([0, 4, 9, 11, 15] if n <= 100 else [0, 16]):
        got = vh.msm(parr, scal, np.array(neg, np.uint8), c=c)
        assert to_pt(got) == want, f"c={c}"


def test_msm_equal_points_and_cancelling_pairs():
    p = o.mul(o.G, 123456789)
    pts = [p] * 50 + [p, o.neg(p)] * 5
    ks = [(1 << 128) - 1 - i for i in range(50)] + [987654321] * 10
    want = _msm_oracle(pts, ks, [0] * 60)
    got = vh.msm(np.stack([pt_bytes(x) for x in pts]), np.stack([fe_bytes(k) for k in ks]))
    assert to_pt(got) == want
    # P and -P with equal scalars only: the identity
    got = vh.msm(np.stack([pt_bytes(p), pt_bytes(o.neg(p))]), np.stack([fe_bytes(o.R_ORDER - 1)] * 2))
    assert to_pt(got) == o.IDENTITY


def _items(b, idx):
    return {k: v[idx] for k, v in b.items()}


def _concat(*bs):
    return {k: np.concatenate([b[k] for b in bs]) for k in bs[0]}


@pytest.mark.parametrize("scheme", SCHEMES)
def test_verdict_of_valid_and_mixed_batches(scheme):
    good = make_batch(scheme, 40, seed=31, n_keys=8, mix=False)
    assert (oracle_verify(scheme, good) == 0).all()
    assert vh.verify_all(scheme, good) == 1
    assert vh.verify_all(scheme, good, seed=bytes(range(32))) == 1
    for c in (8, 11, 15, 16):      # every width the device picks: weights of 135, 131, 134 and 143 bits
        assert vh.verify_all(scheme, good, seed=bytes(range(32)), c=c) == 1
    mixed = make_batch(scheme, 64, seed=32, n_keys=8)
    want = oracle_verify(scheme, mixed)
    assert vh.verify_all(scheme, mixed) == int((want == 0).all())


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("source", ["edge_cases", "torsion_grid"])
def test_verdict_one_item_beside_valid_ones(scheme, source):
    """Every item of the adversarial sets, alone among valid signatures: verdict 1 exactly when its oracle status is 0."""
    b = edge_cases(scheme) if source == "edge_cases" else torsion_grid(scheme, reps=1)
    want = oracle_verify(scheme, b)
    assert vh.verify_all(scheme, b) == int((want == 0).all())
    good = make_batch(scheme, 5, seed=33, n_keys=5, mix=False)
    for i in range(len(want)):
        batch = _concat(_items(good, slice(0, 3)), _items(b, slice(i, i + 1)), _items(good, slice(3, 5)))
        assert vh.verify_all(scheme, batch) == int(want[i] == 0), f"item {i} status {want[i]}"


@pytest.mark.parametrize("scheme", SCHEMES)
def test_cancelling_equations_are_rejected(scheme):
    """u_1 + d and u_2 - d: the two D's sum to O (an unweighted sum would accept), the weighted one does not."""
    b = make_batch(scheme, 6, seed=34, n_keys=6, mix=False)
    if scheme == "vargen":   # the same generator on both items, so that d*Gen cancels
        b["Gen"][1] = b["Gen"][0]
        b = _resign_vargen(b, 1)
        assert (oracle_verify(scheme, b) == 0).all()
    d = 12345
    u1, u2 = int.from_bytes(b["u"][0].tobytes(), "little"), int.from_bytes(b["u"][1].tobytes(), "little")
    b["u"][0] = fe_bytes((u1 + d) % o.R_ORDER)
    b["u"][1] = fe_bytes((u2 - d) % o.R_ORDER)
    want = oracle_verify(scheme, b)
    assert want[0] == 2 and want[1] == 2
    assert vh.verify_all(scheme, b) == 0
    assert vh.verify_all(scheme, b, c=16) == 0


def _resign_vargen(b, i):
    """Item i of a var-gen batch signed again under its (changed) generator."""
    rng = np.random.default_rng(99)
    gen = to_pt(b["Gen"][i])
    sk = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
    k = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
    m = int.from_bytes(b["m"][i].tobytes(), "little")
    PK, R = o.mul(gen, sk), o.mul(gen, k)
    c = o.challenge_vargen(R, PK, gen, m)
    b["PK"][i], b["R"][i], b["u"][i] = pt_bytes(PK), pt_bytes(R), fe_bytes((k - c * sk) % o.R_ORDER)
    return b


def test_cancelling_torsion_is_rejected():
    """R_1 + T and R_2 - T (re-signed so that both prime-order equations hold): the residue test of R_1 + R_2 would pass."""
    t = torsion_generator()
    rng = np.random.default_rng(35)
    rows = []
    for sgn in (1, -1):
        sk = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
        k = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
        m = int.from_bytes(rng.bytes(40), "little") % o.Q
        PK = o.mul(o.G, sk)
        R = o.add(o.mul(o.G, k), t if sgn > 0 else o.neg(t))
        c = o.challenge_single(R, PK, m)
        rows.append({"u": fe_bytes((k - c * sk) % o.R_ORDER), "R": pt_bytes(R), "PK": pt_bytes(PK), "m": fe_bytes(m)})
    b = {key: np.stack([r[key] for r in rows]) for key in ARG_ORDER["single"]}
    assert oracle_verify("single", b).tolist() == [1, 1]
    assert vh.verify_all("single", b) == 0


def test_cofactorless_equation_with_torsion_is_rejected():
    """PK + T and R + c T: u G + c PK == R holds exactly, yet both points carry torsion (InvalidPoint)."""
    t = torsion_generator()
    rng = np.random.default_rng(36)
    sk = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
    m = int.from_bytes(rng.bytes(40), "little") % o.Q
    PK = o.add(o.mul(o.G, sk), t)
    for k in range(1, 200):
        # c depends on R, so search for a nonce whose challenge makes R + c T consistent: R = kG + c T
        for ct in range(8):
            R = o.add(o.mul(o.G, k), o.mul(t, ct))
            c = o.challenge_single(R, PK, m)
            if c % 8 == ct:
                u = (k - c * sk) % o.R_ORDER
                assert o.add(o.mul(o.G, u), o.mul(PK, c)) == R
                b = {"u": fe_bytes(u)[None], "R": pt_bytes(R)[None], "PK": pt_bytes(PK)[None], "m": fe_bytes(m)[None]}
                assert oracle_verify("single", b).tolist() == [1]
                assert vh.verify_all("single", b) == 0
                return
    pytest.fail("no consistent nonce found")

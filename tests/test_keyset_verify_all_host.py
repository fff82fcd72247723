"""The CPU build of csrc/keyset_verdict.h (the batch verdict against a registered key set) against the oracle: the collapsed
sum against the straight per-item sum with the same weights, the verdict against all(status == 0), invalid keys' tables
never read, and the run sums under skew.  No GPU."""
import numpy as np
import pytest

import jjs_oracle as o
import keyset_verdict_hostlib as kv
import verdict_hostlib as vh
from helpers import IDENT, edge_cases, fe_bytes, make_batch, oracle_verify, to_int, to_pt, torsion_grid

KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
SCHEMES = ["single", "double", "vargen"]
SEED = bytes(range(32))


def register(scheme, b):
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in KEYCOLS[scheme]], 1))
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    return [uniq[:, 64 * i:64 * i + 64] for i in range(len(KEYCOLS[scheme]))], inv.reshape(-1).astype(np.uint32)


def weights(seed, item, bits):
    """bv_weights: block `item` of the ChaCha20 keystream; z = words 0-4, z' = words 5-9, cut to `bits`."""
    block = vh.chacha20_block(seed, item & 0xFFFFFFFF, (item >> 32).to_bytes(4, "little") + bytes(8))
    mask = (1 << bits) - 1
    return int.from_bytes(block[:20], "little") & mask, int.from_bytes(block[20:40], "little") & mask


def challenge(scheme, b, i):
    pts = {k: to_pt(b[k][i]) for k in b if k not in ("u", "m")}
    m = to_int(b["m"][i])
    if scheme == "single":
        return o.challenge_single(pts["R"], pts["PK"], m)
    if scheme == "double":
        return o.challenge_double(pts["R"], pts["Rp"], pts["PK"], pts["PKp"], m)
    return o.challenge_vargen(pts["R"], pts["PK"], pts["Gen"], m)


def straight_sum(scheme, b, bits, seed=SEED):
    """sum_i z_i (u_i G + c_i PK_i - R_i) (+ the second equation of the double scheme), term by term."""
    acc = o.IDENTITY
    for i in range(len(b["u"])):
        z, zp = weights(seed, i, bits)
        u, c = to_int(b["u"][i]), challenge(scheme, b, i)
        eqs = [(z, o.G if scheme != "vargen" else to_pt(b["Gen"][i]), to_pt(b["PK"][i]), to_pt(b["R"][i]))]
        if scheme == "double":
            eqs.append((zp, o.G_NUMS, to_pt(b["PKp"][i]), to_pt(b["Rp"][i])))
        for w, gen, pk, r in eqs:
            d = o.add(o.add(o.mul(gen, u), o.mul(pk, c)), o.neg(r))
            acc = o.add(acc, o.mul(d, w))
    return acc


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("c", [0, 8, 13, 16])
def test_collapsed_sum_equals_the_straight_sum(scheme, c):
    """Repeated keys, some failing equations (the sum is then not O), pinned weights."""
    b = make_batch(scheme, 24, seed=41 + c, n_keys=5, mix=False)
    for i in (2, 9, 10):
        b["u"][i] = fe_bytes((to_int(b["u"][i]) + 7 + i) % o.R_ORDER)
    assert sorted(set(oracle_verify(scheme, b).tolist())) == [0, 2]
    keys, idx = register(scheme, b)
    got = kv.verify_all(scheme, keys, idx, b, seed=SEED, c=c)
    want = straight_sum(scheme, b, got["z_bits"])
    assert want != o.IDENTITY
    assert to_pt(got["total"]) == want
    assert got["verdict"] == 0
    good = make_batch(scheme, 24, seed=41 + c, n_keys=5, mix=False)
    got = kv.verify_all(scheme, keys, idx, good, seed=SEED, c=c)
    assert to_pt(got["total"]) == o.IDENTITY == straight_sum(scheme, good, got["z_bits"])
    assert got["verdict"] == 1


def _items(b, idx):
    return {k: v[idx] for k, v in b.items()}


def _concat(*bs):
    return {k: np.concatenate([b[k] for b in bs]) for k in bs[0]}


@pytest.mark.parametrize("scheme", SCHEMES)
def test_verdict_of_valid_and_mixed_batches(scheme):
    good = make_batch(scheme, 40, seed=31, n_keys=8, mix=False)
    assert (oracle_verify(scheme, good) == 0).all()
    keys, idx = register(scheme, good)
    assert kv.verify_all(scheme, keys, idx, good)["verdict"] == 1
    for c in range(8, 17):
        assert kv.verify_all(scheme, keys, idx, good, seed=SEED, c=c)["verdict"] == 1, c
    mixed = make_batch(scheme, 64, seed=32, n_keys=8)
    keys, idx = register(scheme, mixed)
    want = oracle_verify(scheme, mixed)
    assert kv.verify_all(scheme, keys, idx, mixed)["verdict"] == int((want == 0).all())


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("source", ["edge_cases", "torsion_grid"])
def test_verdict_one_item_beside_valid_ones(scheme, source):
    """Every item of the adversarial sets, its key registered, alone among valid signatures: verdict 1 exactly when its
    oracle status is 0."""
    b = edge_cases(scheme) if source == "edge_cases" else torsion_grid(scheme, reps=1)
    want = oracle_verify(scheme, b)
    good = make_batch(scheme, 5, seed=33, n_keys=3, mix=False)
    keys, idx = register(scheme, _concat(good, b))
    assert kv.verify_all(scheme, keys, idx, _concat(good, b))["verdict"] == int((want == 0).all())
    for i in range(len(want)):
        sel = np.array([0, 1, 2, 5 + i, 3, 4])
        got = kv.verify_all(scheme, keys, idx[sel], _items(_concat(good, b), sel))
        assert got["verdict"] == int(want[i] == 0), f"item {i} status {want[i]}"


def _with_bad_keys(scheme, b, keys, idx):
    """Two more keys: the identity (status 1) and a non-canonical coordinate (status 3)."""
    ident = keys[0][:1].copy(); ident[0] = IDENT
    nc = keys[0][:1].copy(); nc[0, :32] = fe_bytes(o.Q)
    return [np.concatenate([k, ident, nc]) if i == 0 else np.concatenate([k, k[:1], k[:1]]) for i, k in enumerate(keys)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", ["index_beyond_the_set", "index_max", "key_status_1", "key_status_3"])
def test_bad_index_and_invalid_keys_fail_the_batch(scheme, case):
    b = make_batch(scheme, 20, seed=23, n_keys=4, mix=False)
    keys, idx = register(scheme, b)
    keys = _with_bad_keys(scheme, b, keys, idx)
    nk = len(keys[0])
    assert kv.verify_all(scheme, keys, idx, b)["verdict"] == 1
    idx[7] = {"index_beyond_the_set": nk, "index_max": 0xFFFFFFFF, "key_status_1": nk - 2, "key_status_3": nk - 1}[case]
    got = kv.verify_all(scheme, keys, idx, b)
    assert got["key_status"][-2] == 1 and got["key_status"][-1] == 3
    assert got["verdict"] == 0


@pytest.mark.parametrize("scheme", SCHEMES)
def test_tables_of_invalid_keys_are_never_read(scheme):
    b = make_batch(scheme, 30, seed=24, n_keys=4, mix=False)
    keys, idx = register(scheme, b)
    keys = _with_bad_keys(scheme, b, keys, idx)
    idx[[3, 11]] = [len(keys[0]) - 2, len(keys[0]) - 1]
    b["u"][5] = fe_bytes((to_int(b["u"][5]) + 1) % o.R_ORDER)         # the sum is not O either
    plain = kv.verify_all(scheme, keys, idx, b, seed=SEED)
    poisoned = kv.verify_all(scheme, keys, idx, b, seed=SEED, poison=True)
    assert plain["verdict"] == poisoned["verdict"] == 0
    np.testing.assert_array_equal(plain["total"], poisoned["total"])
    np.testing.assert_array_equal(plain["key_sums"], poisoned["key_sums"])
    assert to_pt(plain["total"]) != o.IDENTITY


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", ["one_key", "one_item_per_key", "uneven"])
def test_run_sums_under_skew(scheme, shape):
    """S_k against a Python sum mod r: runs longer than a piece (512 items), runs of one item, and a mix that puts run
    boundaries on and off the lines.  The items are 40 signatures repeated (a repeated item is a valid item)."""
    n = 1300
    base = make_batch(scheme, 40, seed=25, n_keys=40, mix=False)
    keys, kidx = register(scheme, base)
    rep = np.arange(n) % 40
    b = _items(base, rep)
    if shape == "one_key":
        # every item under key 0: the signatures of the other keys fail, which does not change the sums' definition
        idx = np.zeros(n, np.uint32)
        for name, col in zip(KEYCOLS[scheme], keys):
            b[name] = np.repeat(col[:1], n, 0)
    elif shape == "one_item_per_key":
        n = 40
        b, idx = base, kidx
    else:
        sizes = [512, 1, 511, 0, 200, 76]                              # runs end on a line, start on one, cross one
        idx = np.repeat(np.arange(len(sizes)), sizes).astype(np.uint32)
        rng = np.random.default_rng(5)
        idx = idx[rng.permutation(n)]
        for name, col in zip(KEYCOLS[scheme], keys):
            b[name] = col[idx]
    got = kv.verify_all(scheme, keys, idx, b, seed=SEED)
    status = oracle_verify(scheme, b)
    assert set(status.tolist()) <= {0, 2}
    want = np.zeros((len(keys), len(keys[0])), object)
    for i in range(n):
        z, zp = weights(SEED, i, got["z_bits"])
        c, u = challenge(scheme, b, i), to_int(b["u"][i])
        want[0, idx[i]] = (want[0, idx[i]] + z * c) % o.R_ORDER
        if scheme == "double":
            want[1, idx[i]] = (want[1, idx[i]] + zp * c) % o.R_ORDER
        if scheme == "vargen":
            want[1, idx[i]] = (want[1, idx[i]] + z * u) % o.R_ORDER
    sums = np.array([[to_int(got["key_sums"][ci, k]) for k in range(len(keys[0]))] for ci in range(len(keys))], object)
    assert (sums == want).all()
    assert got["verdict"] == int((status == 0).all())

"""Cases for signing and key derivation with a SecretKey in the single and double schemes (jjs_sign_fixed*, jjs_public_keys_fixed*,
csrc/sign_fixed.h), shared by the CPU build (test_sign_fixed_host.py) and the device (test_sign_fixed_gpu.py).

`call(double)` is ONE call of 64 items with what it must give.  Its malformed rows stand at lanes 0, 31, 32 and 63 and at 7, 40
and 50:
  sk = r; rnd = r; m = q; sk, rnd, m of 32 x 0xFF, one column each; and one row with all three out of range
Its good edge rows are sk = 0, sk = 1, sk = r - 1, rnd = 0, rnd = r - 1, m = 0 and m = q - 1 (the other columns random), the rest
random rows.  Expected values come from oracle/jjs_oracle.py alone (sign_single_with_rand, sign_double_with_rand, mul, compress,
verify_single, verify_double): a malformed row is status 3 and zero bytes everywhere, a good row the oracle's bytes.  Nothing here
comes from the code under test.  Fixed numpy seed."""
from __future__ import annotations

import functools

import numpy as np

import jjs_oracle as o
from helpers import fe_bytes, pt_bytes, to_int

N = 64
SEED = 1800
PLACES = (0, 31, 32, 63, 7, 40, 50)
KINDS = ("sk=r", "rnd=r", "m=q", "sk=ff", "rnd=ff", "m=ff", "all")
EDGES = (("sk", 0), ("sk", 1), ("sk", o.R_ORDER - 1), ("rnd", 0), ("rnd", o.R_ORDER - 1), ("m", 0), ("m", o.Q - 1))
EDGE_PLACES = (1, 2, 3, 30, 33, 61, 62)
FF = np.full(32, 0xFF, np.uint8)
OUTPUTS = ("u", "R", "Rp", "PK", "PKp", "sig_w", "pk_w")
KEYED_KEYS = ("random", "0", "r-1", "unusable")


def _rand_below(rng, mod):
    return int.from_bytes(rng.bytes(48), "little") % mod


def outputs_of(double):
    return tuple(k for k in OUTPUTS if double or k not in ("Rp", "PKp"))


@functools.lru_cache(maxsize=None)
def signed(double: bool, sk: int, rnd: int, m: int):
    """The oracle's rows of one good item: {u, R, [Rp,] PK, [PKp,] sig_w, pk_w} as uint8 arrays, and the verification status."""
    PK = o.mul(o.G, sk)
    if double:
        u, R, Rp = o.sign_double_with_rand(sk, rnd, m)
        PKp = o.mul(o.G_NUMS, sk)
        rows = dict(u=fe_bytes(u), R=pt_bytes(R), Rp=pt_bytes(Rp), PK=pt_bytes(PK), PKp=pt_bytes(PKp),
                    sig_w=np.frombuffer(o.le32(u) + o.compress(R) + o.compress(Rp), np.uint8),
                    pk_w=np.frombuffer(o.compress(PK) + o.compress(PKp), np.uint8))
        return rows, o.verify_double(u, R, Rp, PK, PKp, m)
    u, R = o.sign_single_with_rand(sk, rnd, m)
    rows = dict(u=fe_bytes(u), R=pt_bytes(R), PK=pt_bytes(PK), sig_w=np.frombuffer(o.le32(u) + o.compress(R), np.uint8),
                pk_w=np.frombuffer(o.compress(PK), np.uint8))
    return rows, o.verify_single(u, R, PK, m)


@functools.lru_cache(maxsize=None)
def key_rows(double: bool, sk: int):
    """The oracle's key rows of sk: {PK, [PKp,] pk_w}."""
    PK = o.mul(o.G, sk)
    if not double:
        return dict(PK=pt_bytes(PK), pk_w=np.frombuffer(o.compress(PK), np.uint8))
    PKp = o.mul(o.G_NUMS, sk)
    return dict(PK=pt_bytes(PK), PKp=pt_bytes(PKp), pk_w=np.frombuffer(o.compress(PK) + o.compress(PKp), np.uint8))


def widths(double):
    return dict(u=32, R=64, Rp=64, PK=64, PKp=64, sig_w=96 if double else 64, pk_w=64 if double else 32)


class Call:
    """One call: sk (n or 1, 32), rnd, m (n, 32), the expected outputs `want` ({name: array}, the key outputs of sk's row count) and
    status; `verify`: the oracle's verification status of every good row's signature (-1 for a malformed row)."""

    def __init__(self, double, sk, rnd, m, want, status, verify, labels):
        self.double, self.sk, self.rnd, self.m, self.want, self.status, self.verify, self.labels = double, sk, rnd, m, want, status, verify, labels

    @property
    def n(self):
        return len(self.rnd)


@functools.lru_cache(maxsize=None)
def call(double: bool) -> Call:
    rng = np.random.default_rng(SEED + int(double))
    vals = [dict(sk=_rand_below(rng, o.R_ORDER), rnd=_rand_below(rng, o.R_ORDER), m=_rand_below(rng, o.Q), kind=None, label="random") for _ in range(N)]
    for place, (col, v) in zip(EDGE_PLACES, EDGES):
        vals[place][col] = v
        vals[place]["label"] = "%s=%s" % (col, {0: "0", 1: "1", o.R_ORDER - 1: "r-1", o.Q - 1: "q-1"}[v])
    cols = {c: np.stack([fe_bytes(v[c]) for v in vals]) for c in ("sk", "rnd", "m")}
    for place, kind in zip(PLACES, KINDS):
        vals[place]["kind"] = vals[place]["label"] = kind
        for c, bound in (("sk", o.R_ORDER), ("rnd", o.R_ORDER), ("m", o.Q)):
            if kind in (c + "=r", c + "=q", "all"):
                cols[c][place] = fe_bytes(bound)
            elif kind == c + "=ff":
                cols[c][place] = FF
    w = widths(double)
    want = {k: np.zeros((N, w[k]), np.uint8) for k in outputs_of(double)}
    status, verify = np.zeros(N, np.uint8), np.full(N, -1, np.int64)
    for i, v in enumerate(vals):
        if v["kind"] is not None:
            status[i] = 3
            continue
        rows, verify[i] = signed(double, v["sk"], v["rnd"], v["m"])
        for k in want:
            want[k][i] = rows[k]
    return Call(double, cols["sk"], cols["rnd"], cols["m"], want, status, verify, ["%d %s" % (i, v["label"]) for i, v in enumerate(vals)])


def keyed_key(which: str) -> int:
    return {"random": 0x0123456789ABCDEF0FEDCBA987654321 * 0x1F3D5B79 % o.R_ORDER, "0": 0, "r-1": o.R_ORDER - 1, "unusable": o.R_ORDER}[which]


def keyed_call(double: bool, which: str, n: int, seed: int = SEED + 7):
    """sk (1 row), rnd, m of a call of n items under ONE key: `which` of KEYED_KEYS.  Row 0 has rnd = r (a malformed item under a
    usable key: the key rows do not depend on it) when n > 2, row 1 rnd = 0; the rest random."""
    rng = np.random.default_rng(seed + n)
    sk = fe_bytes(keyed_key(which)).reshape(1, 32)
    rnd = np.stack([fe_bytes(_rand_below(rng, o.R_ORDER)) for _ in range(n)])
    m = np.stack([fe_bytes(_rand_below(rng, o.Q)) for _ in range(n)])
    if n > 2:
        rnd[0] = fe_bytes(o.R_ORDER)
        rnd[1] = fe_bytes(0)
    return sk, rnd, m


def oracle_rows(double, sk, rnd, m, rows):
    """{row: {name: bytes}} of the given (good) rows of a call; sk of n rows or of one."""
    return {i: signed(double, to_int(sk[i if len(sk) > 1 else 0]), to_int(rnd[i]), to_int(m[i]))[0] for i in rows}


def kat(reference_kat):
    """The reference's own bytes (tests/golden/reference_kat.json, seed 2321), the draws in the order tests/test_oracle_kat.py
    reproduces them (single: sk, m, then the nonce's draw; double: the same order from a fresh generator), the bytes they must
    give, and the three (secret key, public key) pairs of multisig_kat for the derivation."""
    v = reference_kat["serde_base58"]
    rng = o.StdRng(v["seed"])
    sk = rng.random_fr()
    m = rng.random_fq()
    rnd = rng.random_fr()
    rng = o.StdRng(v["seed"])
    assert (rng.random_fr(), rng.random_fq()) == (sk, m)
    rnd_double = rng.random_fr()
    mk = reference_kat["multisig_kat"]
    return dict(secret=o.b58decode(v["serde_secret_key"]), public=o.b58decode(v["serde_public_key"]),
                public_double=o.b58decode(v["serde_public_key_double"]), signature=o.b58decode(v["serde_signature"]),
                signature_double=o.b58decode(v["serde_signature_double"]), sk=fe_bytes(sk), m=fe_bytes(m), rnd=fe_bytes(rnd),
                rnd_double=fe_bytes(rnd_double),
                pairs=[(fe_bytes(int(s)), bytes.fromhex(p)) for s, p in zip(mk["secret_keys"], mk["public_keys"])])


def check(got, c: Call, label="", skip=()):
    """got: {name: array, "status": array} of the call; byte for byte."""
    assert got["status"].tolist() == c.status.tolist(), (label, "status", got["status"].tolist(), c.status.tolist())
    for name, want in c.want.items():
        if name in skip:
            continue
        assert got[name].shape == want.shape, (label, name, got[name].shape)
        bad = np.nonzero((got[name] != want).any(1))[0]
        assert not len(bad), (label, name, [c.labels[i] for i in bad[:6]])

"""Cases for var-generator signing and key derivation with the generator as a point (jjs_sign_vargen_pt*, jjs_public_keys_vargen*,
csrc/sign_vargen.h), shared by the CPU build (test_sign_vargen_pt_host.py) and the device (test_sign_vargen_pt_gpu.py).

`call(fmt)` is ONE call of 64 items in the format `fmt`, with what it must give.  Its good rows walk these generators
  k * G; points decoded from counter encodings (arbitrary curve points, most with a torsion part); P + T for each of the eight
  torsion points T; the identity (0, 1); (0, -1); a point of order 4; a point of order 8
three times over, under sk in {0, 1, r - 1, random}, rnd in {0, r - 1, random} and m in {0, q - 1, random}.  Its malformed rows
stand at lanes 0, 31, 32 and 63 (and, where a format has more kinds than four, at 7, 40 and 50):
  every format  sk = r; rnd = r; m = q
  affine        generator u = q; the generator (1, 1), off the curve
  extended      U = q; (1, 1) with Z = 1; Z = 0; Z = q
  wire          v >= q; u = 0 with the sign bit; an encoding with no square root
Expected values come from oracle/jjs_oracle.py alone (sign_vargen_with_rand, mul, compress, verify_vargen): a malformed row is
status 3 and zero bytes everywhere, a good row the oracle's bytes.  Nothing here comes from the code under test.  Fixed numpy seed."""
from __future__ import annotations

import functools

import numpy as np

import jjs_oracle as o
from helpers import fe_bytes, pt_bytes, to_int, torsion_generator

FORMATS = ("affine", "ext", "wire")
FORMAT_CODE = {"affine": 0, "ext": 1, "wire": 2}
GEN_WIDTH = {"affine": 64, "ext": 96, "wire": 32}
N = 64
SEED = 1700
FIRST_PLACES = (0, 31, 32, 63)
MORE_PLACES = (7, 40, 50)
COMMON_KINDS = ("sk=r", "rnd=r", "m=q")
KINDS = {"affine": COMMON_KINDS + ("u=q", "off-curve"),
         "ext": COMMON_KINDS + ("u=q", "off-curve", "Z=0", "Z=q"),
         "wire": COMMON_KINDS + ("v>=q", "u=0 signed", "no root")}


def _rand_below(rng, mod):
    return int.from_bytes(rng.bytes(48), "little") % mod


@functools.lru_cache(maxsize=None)
def generators():
    """[(label, point, torsion_free_and_not_identity)]"""
    t8 = torsion_generator()
    base = o.mul(o.G, 0x1234567)
    gens = [("%d*G" % k, o.mul(o.G, k)) for k in (1, 5, o.R_ORDER - 1)]
    v, found = 2, 0
    while found < 4:                                     # counter encodings that decode
        p = o.decompress(o.le32(v))
        if p is not None:
            gens.append(("decoded v=%d" % v, p))
            found += 1
        v += 1
    gens += [("P+%dT" % k, o.add(base, o.mul(t8, k))) for k in range(8)]
    gens += [("identity", o.IDENTITY), ("(0,-1)", (0, o.Q - 1)), ("order 4", o.mul(t8, 2)), ("order 8", t8)]
    assert gens[-3][1] == o.ORDER2 and o.mul(gens[-2][1], 2) == o.ORDER2 and o.mul(t8, 4) == o.ORDER2
    assert all(o.is_on_curve(p) for _, p in gens)
    return [(label, p, o.point_is_valid(p)) for label, p in gens]


def no_root_encoding() -> bytes:
    v = 2
    while o.decompress(o.le32(v)) is not None:
        v += 1
    return o.le32(v)


def to_ext_row(p, z: int) -> np.ndarray:
    return np.concatenate([fe_bytes(p[0] * z % o.Q), fe_bytes(p[1] * z % o.Q), fe_bytes(z)])


def gen_column(points, fmt, rng=None) -> np.ndarray:
    """The generator column of `points` (affine tuples) in the format: extended with random Z (the first rows Z = 1, q - 1, 2)."""
    if fmt == "affine":
        return np.stack([pt_bytes(p) for p in points])
    if fmt == "wire":
        return np.stack([np.frombuffer(o.compress(p), np.uint8) for p in points])
    rng = rng or np.random.default_rng(SEED + 1)
    zs = [1, o.Q - 1, 2] + [1 + _rand_below(rng, o.Q - 1) for _ in points]
    return np.stack([to_ext_row(p, zs[i]) for i, p in enumerate(points)])


class Call:
    """One call: sk, rnd, m (n, 32), Gen (n_gen, width of the format), and the expected u, R, PK, Gen_out, status; `verify`: the
    oracle's verify_vargen status of every good row's signature (-1 for a malformed row)."""

    def __init__(self, fmt, sk, Gen, rnd, m, want, verify, labels):
        self.fmt, self.sk, self.Gen, self.rnd, self.m = fmt, sk, Gen, rnd, m
        self.u, self.R, self.PK, self.Gen_out, self.status = want
        self.verify, self.labels = verify, labels

    @property
    def n(self):
        return len(self.sk)


@functools.lru_cache(maxsize=None)
def _signed(sk: int, gen, rnd: int, m: int):
    u, R = o.sign_vargen_with_rand(sk, gen, rnd, m)
    PK = o.mul(gen, sk)
    return u, R, PK, o.verify_vargen(u, R, PK, gen, m)


@functools.lru_cache(maxsize=None)
def call(fmt: str) -> Call:
    rng = np.random.default_rng(SEED)
    gens = generators()
    kinds = KINDS[fmt]
    places = dict(zip(FIRST_PLACES + MORE_PLACES, kinds))
    sks = [0, 1, o.R_ORDER - 1, _rand_below(rng, o.R_ORDER)]
    rnds = [0, o.R_ORDER - 1, _rand_below(rng, o.R_ORDER)]
    ms = [0, o.Q - 1, _rand_below(rng, o.Q)]
    rows, good = [], 0
    for i in range(N):
        label, p, _ = gens[good % len(gens)]
        rep = good // len(gens)
        # the three visits of a generator see three different combinations; (good + rep) walks the scalars against each other
        row = dict(sk=sks[(good + rep) % 4], rnd=rnds[(good + 2 * rep) % 3], m=ms[(good // 3 + rep) % 3], gen=p, label=label, kind=places.get(i))
        if row["kind"] is None:
            good += 1
        rows.append(row)
    assert good >= 3 * len(gens) - 2, "every generator is visited about three times"
    sk = np.stack([fe_bytes(o.R_ORDER if r["kind"] == "sk=r" else r["sk"]) for r in rows])
    rnd = np.stack([fe_bytes(o.R_ORDER if r["kind"] == "rnd=r" else r["rnd"]) for r in rows])
    m = np.stack([fe_bytes(o.Q if r["kind"] == "m=q" else r["m"]) for r in rows])
    Gen = gen_column([r["gen"] for r in rows], fmt, np.random.default_rng(SEED + 2))
    for i, r in enumerate(rows):
        k = r["kind"]
        if k == "u=q":
            Gen[i, :32] = fe_bytes(o.Q)
        elif k == "off-curve":
            Gen[i] = pt_bytes((1, 1)) if fmt == "affine" else to_ext_row((1, 1), 1)
        elif k == "Z=0":
            Gen[i, 64:] = 0
        elif k == "Z=q":
            Gen[i, 64:] = fe_bytes(o.Q)
        elif k == "v>=q":
            Gen[i] = fe_bytes(o.Q + 1)
        elif k == "u=0 signed":
            b = bytearray(o.compress(o.IDENTITY)); b[31] |= 0x80
            Gen[i] = np.frombuffer(bytes(b), np.uint8)
        elif k == "no root":
            Gen[i] = np.frombuffer(no_root_encoding(), np.uint8)
    assert not o.is_on_curve((1, 1))
    u, R, PK, G_out = np.zeros((N, 32), np.uint8), np.zeros((N, 64), np.uint8), np.zeros((N, 64), np.uint8), np.zeros((N, 64), np.uint8)
    status, verify = np.zeros(N, np.uint8), np.full(N, -1, np.int64)
    for i, r in enumerate(rows):
        if r["kind"] is not None:
            status[i] = 3
            continue
        uu, RR, PP, vv = _signed(r["sk"], r["gen"], r["rnd"], r["m"])
        u[i], R[i], PK[i], G_out[i], verify[i] = fe_bytes(uu), pt_bytes(RR), pt_bytes(PP), pt_bytes(r["gen"]), vv
    labels = ["%s sk=%x.. (%s)" % (r["label"], r["sk"] & 0xFFFF, r["kind"] or "good") for r in rows]
    return Call(fmt, sk, Gen, rnd, m, (u, R, PK, G_out, status), verify, labels)


def expected_verify_by_generator():
    """What verify_vargen says about a signature under each generator with sk != 0: 0 for a prime-order generator, 1 (InvalidPoint)
    for the identity, small-order generators and generators with a torsion part -- asserted against the oracle's own answers by
    the tests that use `Call.verify`."""
    return {label: (0 if valid else 1) for label, _, valid in generators()}


SHARED_GENERATORS = ("5*G", "P+3T", "identity")


def shared_call(which: str, n: int, fmt: str = "affine", seed: int = SEED + 7):
    """sk, Gen (1 row), rnd, m of a call of n items under ONE generator: `which` a label of generators(), or "unusable" (u = q;
    extended Z = 0; wire an encoding with no square root).  Scalars: row 0 sk = 0, row 1 sk = r - 1, the rest random."""
    rng = np.random.default_rng(seed + n)
    if which == "unusable":
        p = o.mul(o.G, 5)
    else:
        p = dict((label, q) for label, q, _ in generators())[which]
    Gen = gen_column([p], fmt, np.random.default_rng(seed))
    if which == "unusable":
        if fmt == "affine":
            Gen[0, :32] = fe_bytes(o.Q)
        elif fmt == "ext":
            Gen[0, 64:] = 0
        else:
            Gen[0] = np.frombuffer(no_root_encoding(), np.uint8)
    sk = np.stack([fe_bytes(_rand_below(rng, o.R_ORDER)) for _ in range(n)])
    sk[0] = fe_bytes(0)
    if n > 1:
        sk[1] = fe_bytes(o.R_ORDER - 1)
    rnd = np.stack([fe_bytes(_rand_below(rng, o.R_ORDER)) for _ in range(n)])
    m = np.stack([fe_bytes(_rand_below(rng, o.Q)) for _ in range(n)])
    return sk, Gen, rnd, m, p


def oracle_rows(sk, p, rnd, m, rows):
    """{row: (u, R, PK) bytes} of the given rows of a call under the generator p (an affine tuple)."""
    out = {}
    for i in rows:
        uu, RR = o.sign_vargen_with_rand(to_int(sk[i]), p, to_int(rnd[i]), to_int(m[i]))
        out[i] = (fe_bytes(uu), pt_bytes(RR), pt_bytes(o.mul(p, to_int(sk[i]))))
    return out


def kat(reference_kat):
    """The reference's own bytes (tests/golden/reference_kat.json, seed 2321): the 64 bytes of serde_secret_key_var_gen, the draw
    behind serde_signature_var_gen as tests/test_oracle_kat.py reproduces it (sk, the generator's scalar, m, then the nonce's
    draw), and the bytes they must give."""
    v = reference_kat["serde_base58"]
    rng = o.StdRng(v["seed"])
    rng.random_fr(); rng.random_fr()
    m = rng.random_fq()
    rnd = rng.random_fr()
    return dict(secret=o.b58decode(v["serde_secret_key_var_gen"]), public=o.b58decode(v["serde_public_key_var_gen"]),
                signature=o.b58decode(v["serde_signature_var_gen"]), m=fe_bytes(m), rnd=fe_bytes(rnd))


def check(got, c: Call, label=""):
    """got: (u, R, PK, Gen_out, status) of the call; byte for byte."""
    u, R, PK, G_out, st = got
    assert st.tolist() == c.status.tolist(), (label, "status", st.tolist(), c.status.tolist())
    for name, a, b in (("u", u, c.u), ("R", R, c.R), ("PK", PK, c.PK), ("Gen_out", G_out, c.Gen_out)):
        bad = np.nonzero((a != b).any(1))[0]
        assert not len(bad), (label, name, [(int(i), c.labels[i]) for i in bad[:6]])

"""tools/edgecheck on the device, every output checked against Python big integers: the values and the output bounds the
callers rely on, not a comparison with the host build.  The code under test is what only the device runs: the generated
blocks in every copy (mont_mul_call, mont_mul_inl, fq_mul_hot, fq_mul_chain, the squares, fq_sqr_plus_const, the Hades
linear layer), the canonical form behind fq_to_words / fq_is_zero / fq_eq, the cooperative permutation (eight lanes) and the
quad doubling (four lanes).  Inputs sit at the edges of the static bounds of each template instantiation: limbs at
L * 2^29 - 1, values just below A q, multiples of q and their neighbours, values in [q, 2q), zeros.  The binary runs once,
in a subprocess with a time limit; each record is one launch, and most end in a partly filled wave."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import jjs_oracle as o
from helpers import const_table, edge_limb_vectors, limbs_val

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "jubjub_schnorr_amd", "tools")
SRC, EXE = os.path.join(TOOLS, "edgecheck.hip"), os.path.join(TOOLS, "edgecheck")
Q = o.Q
RP = 1 << 261
RINV = pow(RP, -1, Q)
INV29 = pow(1 << 29, -1, Q)
M29 = (1 << 29) - 1

with open(SRC) as _f:
    _TEXT = _f.read()
KIND = {k: i + 1 for i, k in enumerate(re.findall(r"\bK_\w+", re.search(r"enum Kind \{(.*?)\}", _TEXT, re.S).group(1)))}
CLASSES = {name: [tuple(int(v) for v in c.split(",")) for c in re.findall(r"X\(([^)]*)\)", body)]
           for name, body in re.findall(r"#define (\w+)_CLASSES\(X\)(.*)", _TEXT)}
OUT_WORDS = {"K_MUL_CALL": 9, "K_MUL_INL": 9, "K_MUL_HOT": 9, "K_MUL_CHAIN": 9, "K_SQR_CALL": 9, "K_SQR_INL": 9, "K_SQR_HOT": 9,
             "K_SQR_PLUS_CONST": 9, "K_SQR_CHAIN": 9, "K_HADES_MATRIX": 45, "K_LINCOMB": 45, "K_TO_WORDS": 8, "K_IS_ZERO": 1,
             "K_EQ": 1, "K_PERMUTE": 45, "K_PERMUTE_COOP": 8 * 45, "K_DOUBLE": 36, "K_DOUBLE_QUAD": 4 * 45, "K_ADD_NIELS": 36}
HANKEL = const_table("JJS_HS_HANKEL")
HADES_CONSTS = const_table("JJS_HS_RC_FULL") + const_table("JJS_HS_KAPPA")
MU = const_table("JJS_HS_MU")
D2 = limbs_val(const_table("JJS_D2")) * RINV % Q
ONE = [1] + [0] * 8


def limbs(x):
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def spread(l, L):
    """the same value with limbs raised towards L * 2^29 - 1 by borrowing from the next limb"""
    l = list(l)
    for i in range(8):
        t = min(L - 1, l[i + 1])
        l[i] += t << 29
        l[i + 1] -= t
    return l


def plain(l):
    return limbs_val(l) * RINV % Q


def edge(rng, n, L, A):
    return [list(map(int, r)) for r in edge_limb_vectors(rng, n, L, A)]


def multiples(L, A):
    """every k q below A q and its neighbours; spread over wider limbs when L > 1"""
    out = []
    for k in range(A):
        for d in (-1, 0, 1):
            if 0 <= k * Q + d < A * Q:
                out.append(limbs(k * Q + d))
                if L > 1:
                    out.append(spread(limbs(k * Q + d), L))
    return out


def plus_const(rng, n):
    """(normalised fe_n at its edges) + each Hades constant, limb by limb: the operands of fq_sqr_plus_const"""
    ns = edge(rng, n, 1, 2)
    return [[x[i] + c[i] for i in range(9)] for c in HADES_CONSTS for x in ns]


def at_bounds(row, ops):
    """(some operand has a limb at L * 2^29 - 1, some operand's value lies within 2^232 of A q)"""
    lim = any(any(x == (L << 29) - 1 for x in row[off:off + 9]) for off, L, A in ops)
    val = any(limbs_val(row[off:off + 9]) > A * Q - (1 << 232) for off, L, A in ops)
    return lim, val


def record(name, kind, cls, rows, ops=(), meta=None):
    la, aa, lb, ab = (cls[0], cls[1], 1, cls[2]) if len(cls) == 3 else (tuple(cls) + (0, 0, 0, 0))[:4]
    c = KIND[kind] << 24 | la << 20 | aa << 12 | lb << 8 | ab
    flags = [at_bounds(r, ops) for r in rows]
    return {"name": name, "kind": kind, "code": c, "rows": rows, "meta": meta, "limb_edges": sum(f[0] for f in flags),
            "value_edges": sum(f[1] for f in flags)}


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def product_records(rng):
    recs, mul_rows, mul_ops = [], [], []
    for kind, classes in (("K_MUL_HOT", CLASSES["MUL_HOT"]), ("K_MUL_CHAIN", CLASSES["MUL_CHAIN"])):
        for la, aa, lb, ab in classes:
            a, b = edge(rng, 320, la, aa), edge(rng, 320, lb, ab)
            if (lb, ab) == (1, 1):                   # the product with the constant 1 of fq_canon_limbs
                a += multiples(la, aa)
                b = [ONE if i % 5 == 0 else y for i, y in enumerate(b)] + [ONE] * (len(a) - len(b))
            if (la, aa) == (1, 1):
                b += multiples(lb, ab)
                a = [ONE if i % 5 == 0 else x for i, x in enumerate(a)] + [ONE] * (len(b) - len(a))
            if (la, aa, lb, ab) == (2, 3, 2, 3):      # the cooperative S-box: x * x and x * mu, x = lane + constant
                xs = plus_const(rng, 4)
                a += xs + xs
                b += xs + [MU[i % 60] for i in range(len(xs))]
            if (la, aa, lb, ab) == (1, 2, 2, 3):
                xs = plus_const(rng, 4)
                a += edge(rng, len(xs), 1, 2)
                b += xs
            ops = ((0, la, aa), (9, lb, ab))
            rows = [x + y for x, y in zip(a, b)]
            recs.append(record("%s%s" % (kind[2:].lower(), (la, aa, lb, ab)), kind, (la, aa, lb, ab), rows, ops))
            mul_rows += rows
            mul_ops += [ops] * len(rows)
    for kind in ("K_MUL_CALL", "K_MUL_INL"):
        r = record(kind[2:].lower(), kind, (), mul_rows)
        f = [at_bounds(row, ops) for row, ops in zip(mul_rows, mul_ops)]
        r["limb_edges"], r["value_edges"] = sum(x[0] for x in f), sum(x[1] for x in f)
        recs.append(r)
    sq_rows, sq_ops = [], []
    for la, aa in CLASSES["SQR_HOT"]:
        rows = edge(rng, 320, la, aa)
        recs.append(record("sqr_hot%s" % ((la, aa),), "K_SQR_HOT", (la, aa), rows, ((0, la, aa),)))
        sq_rows += rows
        sq_ops += [((0, la, aa),)] * len(rows)
    for kind in ("K_SQR_CALL", "K_SQR_INL"):
        r = record(kind[2:].lower(), kind, (), sq_rows)
        f = [at_bounds(row, ops) for row, ops in zip(sq_rows, sq_ops)]
        r["limb_edges"], r["value_edges"] = sum(x[0] for x in f), sum(x[1] for x in f)
        recs.append(r)
    xs = plus_const(rng, 24)
    for la, aa in CLASSES["SQR_PLUS_CONST"]:
        assert (la, aa) == (2, 3)
        recs.append(record("sqr_plus_const%s" % ((la, aa),), "K_SQR_PLUS_CONST", (la, aa), xs, ((0, la, aa),)))
    for la, aa in CLASSES["SQR_CHAIN"]:
        rows = xs if (la, aa) == (2, 3) else edge(rng, 320, la, aa)
        recs.append(record("sqr_chain%s" % ((la, aa),), "K_SQR_CHAIN", (la, aa), rows, ((0, la, aa),)))
    return recs


def hankel_residue_states(rng, n):
    """states whose first column of row i sums to 0, 1, 2, -2 or -1 mod 2^29 (the rounding of the first quotient digit)"""
    inv = pow(HANKEL[3], -1, 1 << 29)
    out = []
    base = edge(rng, 5 * n, 1, 2)
    for s in range(n):
        t = [list(base[5 * s + j]) for j in range(5)]
        i, r = s % 4, (0, 1, 2, M29 - 1, M29)[s % 5]
        rest = sum(HANKEL[i + k] * t[k][0] for k in range(5) if k != 3 - i)
        t[3 - i][0] = (r - rest) * inv % (1 << 29)
        if limbs_val(t[3 - i]) < 2 * Q:
            out.append(sum(t, []))
    return out


def linear_records(rng):
    pool = edge(rng, 5 * 1500, 1, 2)
    rows = [sum(pool[5 * s:5 * s + 5], []) for s in range(1500)]
    rows += [[0] * 45, limbs(2 * Q - 1) * 5, limbs(Q) * 5] + hankel_residue_states(rng, 200)
    ops = tuple((9 * j, 1, 2) for j in range(5))
    return [record("hades_matrix", "K_HADES_MATRIX", (), rows, ops), record("lincomb_small<5>", "K_LINCOMB", (), rows, ops)]


def canonical_records(rng):
    recs = []
    for kind, classes in (("K_TO_WORDS", CLASSES["TO_WORDS"]), ("K_IS_ZERO", CLASSES["IS_ZERO"])):
        for L, A in classes:
            rows = edge(rng, 256, L, A) + multiples(L, A)
            recs.append(record("%s%s" % (kind[2:].lower(), (L, A)), kind, (L, A), rows, ((0, L, A),)))
    for la, aa, ab in CLASSES["EQ"]:
        b = edge(rng, 512, 1, ab)
        a = []
        for k, y in enumerate(b):
            v = limbs_val(y) % Q + (k % aa) * Q + (0, 1, -1, 0)[k % 4]
            a.append(spread(limbs(v), la) if 0 <= v < aa * Q else limbs(limbs_val(y) % Q))
        a[3::8] = edge(rng, len(a[3::8]), la, aa)        # unrelated values
        rows = [x + y for x, y in zip(a, b)]
        recs.append(record("eq%s" % ((la, aa, ab),), "K_EQ", (la, aa, ab), rows, ((0, la, aa), (9, 1, ab))))
    return recs


def permute_records(rng, prng):
    n = 320
    pool = edge(rng, 5 * n, 1, 2)
    states = [pool[5 * s:5 * s + 5] for s in range(n)]
    for s in range(0, n, 4):
        states[s + 1] = [limbs(Q + prng.randrange(Q)) for _ in range(5)]                            # in [q, 2q)
        states[s + 2][s % 5] = [0] * 9
    states += [[[0] * 9] * 5, [limbs(Q)] * 5, [limbs(2 * Q - 1)] * 5, [[M29] * 8 + [limbs(2 * Q - 1)[8]]] * 5]
    rows = [sum(st, []) for st in states]
    ops = tuple((9 * j, 1, 2) for j in range(5))
    return [record("hades_permute", "K_PERMUTE", (), rows, ops), record("hades_permute coop", "K_PERMUTE_COOP", (), rows, ops)]


def mont_rep(x, prng, units=2):
    """a Montgomery representative of the plain value x below units * q"""
    return limbs(x * RP % Q + prng.randrange(units) * Q)


def proj(P, prng):
    """affine P as (X : Y : Z : T) with a random Z, each coordinate c or c + q"""
    u, v = P
    z = prng.randrange(1, Q)
    return sum((mont_rep(c, prng) for c in (u * z % Q, v * z % Q, z, u * v % Q * z % Q)), [])


def point_records(rng, prng):
    pool = edge(rng, 4 * 1000, 1, 2)
    arb = [sum(pool[4 * s:4 * s + 4], []) for s in range(1000)]
    arb += [[0] * 36, limbs(2 * Q - 1) * 4, ([M29] * 8 + [limbs(2 * Q - 1)[8]]) * 4]
    pts = [o.mul(o.G, prng.randrange(1, 1 << 64)) for _ in range(48)] + [o.IDENTITY, o.ORDER2]
    curve = [proj(P, prng) for P in pts for _ in range(4)]
    dbl_meta = [None] * len(arb) + [o.add(P, P) for P in pts for _ in range(4)]
    ops = tuple((9 * j, 1, 2) for j in range(4))
    recs = [record("ext_double", "K_DOUBLE", (), arb + curve, ops, dbl_meta),
            record("ext_double_quad", "K_DOUBLE_QUAD", (), arb + curve, ops, dbl_meta)]
    # ext_add_niels: P + N (or P - N) with N's four coordinates at the fe<1, 5> edges, then N = to_niels(Q) of curve points
    npool = edge(rng, 4 * 1000, 1, 5)
    rows = [arb[s % len(arb)] + sum(npool[4 * s:4 * s + 4], []) + [s & 1] for s in range(1000)]
    meta = [None] * len(rows)
    for s in range(256):
        P, Q2 = pts[s % len(pts)], pts[(7 * s + 3) % len(pts)]
        q2 = proj(Q2, prng)
        X, Y, Z, T = (plain(q2[9 * j:9 * j + 9]) for j in range(4))
        n = [mont_rep(c, prng, 5) for c in ((Y + X) % Q, (Y - X) % Q, Z, T * D2 % Q)]
        neg = s % 3 == 0
        rows.append(proj(P, prng) + sum(n, []) + [int(neg)])
        meta.append(o.add(P, o.neg(Q2) if neg else Q2))
    nops = ops + tuple((36 + 9 * j, 1, 5) for j in range(4))
    recs.append(record("ext_add_niels", "K_ADD_NIELS", (), rows, nops, meta))
    return recs


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_tools()                                       # builds tools/edgecheck when it is missing or stale
    assert os.path.exists(EXE)
    rng, prng = np.random.default_rng(0xED6E), random.Random(0xED6E)
    recs = product_records(rng) + linear_records(rng) + canonical_records(rng) + permute_records(rng, prng) + \
        point_records(rng, prng)
    d = tmp_path_factory.mktemp("edgecheck")
    with open(d / "in.bin", "wb") as f:
        for r in recs:
            f.write(np.array([r["code"], len(r["rows"])], np.uint32).tobytes())
            f.write(np.array(r["rows"], np.uint32).tobytes())
    p = subprocess.run([EXE, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = np.fromfile(d / "out.bin", np.uint32)
    pos = 0
    for r in recs:
        n, w = len(r["rows"]), OUT_WORDS[r["kind"]]
        r["out"] = [list(map(int, x)) for x in out[pos:pos + n * w].reshape(n, w)]
        pos += n * w
        print("%-28s %5d inputs, %5d with a limb at its bound, %5d with the value at its bound"
              % (r["name"], n, r["limb_edges"], r["value_edges"]))
    assert pos == len(out)
    return {r["name"]: r for r in recs}


def pick(dev, *kinds):
    recs = [r for r in dev.values() if r["kind"] in kinds]
    assert recs, kinds
    return recs


def check_fe(l, what):
    """normalised limbs, value below 2q"""
    assert all(x < 1 << 29 for x in l[:8]) and limbs_val(l) < 2 * Q, what


# ---- checks ----------------------------------------------------------------------------------------------------------------
def test_products_at_every_bound_class(dev):
    for r in pick(dev, "K_MUL_CALL", "K_MUL_INL", "K_MUL_HOT", "K_MUL_CHAIN", "K_SQR_CALL", "K_SQR_INL", "K_SQR_HOT",
                  "K_SQR_PLUS_CONST", "K_SQR_CHAIN"):
        square = r["kind"].startswith("K_SQR")
        for row, out in zip(r["rows"], r["out"]):
            a = limbs_val(row[:9])
            b = a if square else limbs_val(row[9:18])
            v = limbs_val(out)
            what = (r["name"], row)
            check_fe(out, what)
            assert v > 0 and v % Q == a * b * RINV % Q, what
            if not square and ONE in (row[:9], row[9:18]):
                assert v <= Q, what                      # fq_canon_limbs: [1, q], q standing for zero


def test_linear_layer_rows(dev):
    m, s = dev["hades_matrix"], dev["lincomb_small<5>"]
    for row, out in zip(m["rows"], m["out"]):
        t = [limbs_val(row[9 * j:9 * j + 9]) for j in range(5)]
        for i in range(5):
            check_fe(out[9 * i:9 * i + 9], (i, row))
            assert limbs_val(out[9 * i:9 * i + 9]) % Q == sum(HANKEL[i + j] * t[j] for j in range(5)) * INV29 % Q, (i, row)
    assert m["out"] == s["out"]             # the asm block and the C++ rows take the same quotient digit: same limbs


def test_canonical_form_and_comparisons(dev):
    for r in pick(dev, "K_TO_WORDS"):
        for row, out in zip(r["rows"], r["out"]):
            assert sum(w << (32 * i) for i, w in enumerate(out)) == plain(row), (r["name"], row)
    for r in pick(dev, "K_IS_ZERO"):
        zeros = 0
        for row, out in zip(r["rows"], r["out"]):
            assert out[0] == int(limbs_val(row) % Q == 0), (r["name"], row)
            zeros += out[0]
        assert zeros >= 2, r["name"]
    for r in pick(dev, "K_EQ"):
        hits = 0
        for row, out in zip(r["rows"], r["out"]):
            assert out[0] == int((limbs_val(row[:9]) - limbs_val(row[9:])) % Q == 0), (r["name"], row)
            hits += out[0]
        assert 0 < hits < len(r["rows"]), r["name"]


def test_permutation_plain_and_cooperative(dev):
    p, c = dev["hades_permute"], dev["hades_permute coop"]
    for row, out, cout in zip(p["rows"], p["out"], c["out"]):
        want = o.hades_permute([plain(row[9 * j:9 * j + 9]) for j in range(5)])
        lanes = [cout[45 * k:45 * k + 45] for k in range(8)]
        assert all(lane == lanes[0] for lane in lanes), row        # all eight lanes end with the same state
        for i in range(5):
            check_fe(out[9 * i:9 * i + 9], ("plain", i, row))
            check_fe(lanes[0][9 * i:9 * i + 9], ("coop", i, row))
            assert plain(out[9 * i:9 * i + 9]) == want[i], ("plain", i, row)
            assert plain(lanes[0][9 * i:9 * i + 9]) == want[i], ("coop", i, row)


def dbl_formula(X, Y, Z, T):
    e, xx, yy, c2 = 2 * X * Y, X * X, Y * Y, 2 * Z * Z
    g, h, f = yy + xx, yy - xx, c2 + xx - yy
    return [e * f % Q, h * g % Q, f * h % Q, g * e % Q]


def add_formula(X, Y, Z, T, ypx, ymx, z, t2d, neg):
    if neg:
        ypx, ymx, t2d = ymx, ypx, -t2d
    a, b, c, d = (Y - X) * ymx, (Y + X) * ypx, T * t2d, 2 * Z * z
    e, f, g, h = b - a, d - c, d + c, b + a
    return [e * f % Q, g * h % Q, f * g % Q, h * e % Q]


def check_point(out, want_affine, what):
    X, Y, Z, T = (plain(out[9 * j:9 * j + 9]) for j in range(4))
    u, v = want_affine
    assert Z != 0 and X == u * Z % Q and Y == v * Z % Q and T * Z % Q == X * Y % Q, what


def test_doubling_plain_and_quad(dev):
    d, qd = dev["ext_double"], dev["ext_double_quad"]
    assert D2 == 2 * o.D % Q
    for row, out, qout, want in zip(d["rows"], d["out"], qd["out"], d["meta"]):
        coords = [plain(row[9 * j:9 * j + 9]) for j in range(4)]
        for j in range(4):
            check_fe(out[9 * j:9 * j + 9], (j, row))
        assert [plain(out[9 * j:9 * j + 9]) for j in range(4)] == dbl_formula(*coords), row
        for lane in range(4):
            q = qout[45 * lane:45 * lane + 45]
            assert q[:36] == out, (lane, row)                                   # bit for bit
            assert q[36:] == out[9 * lane:9 * lane + 9], (lane, row)            # this lane's own product
        if want is not None:
            check_point(out, want, row)


def test_addition_of_cached_points(dev):
    r = dev["ext_add_niels"]
    for row, out, want in zip(r["rows"], r["out"], r["meta"]):
        vals = [plain(row[9 * j:9 * j + 9]) for j in range(8)]
        for j in range(4):
            check_fe(out[9 * j:9 * j + 9], (j, row))
        assert [plain(out[9 * j:9 * j + 9]) for j in range(4)] == add_formula(*vals, row[72]), row
        if want is not None:
            check_point(out, want, row)

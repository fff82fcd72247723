"""Inputs and checks of the scalar-multiplication tests, shared by the CPU build (test_scalar_mul_host.py) and the device
(test_scalar_mul_gpu.py): crafted scalars per window width (4: per-lane tables, 5 and 6: key tables, 16: comb), points of
every class, the records of tools/scalar_stages.h, and the comparison of every output with the Python oracle's big-integer
curve arithmetic (o.mul, o.add, o.neg) -- never with the host build and never with the device.  Every class of case is
counted; CLASS_COUNTS is asserted non-zero class by class, so a change here cannot silently empty one."""
import os
import random
import re

import numpy as np

import jjs_oracle as o
from helpers import fe_bytes, limbs_val, pt_bytes, torsion_generator

Q, R = o.Q, o.R_ORDER
RINV = pow(1 << 261, -1, Q)
D2 = 2 * o.D % Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "scalar_stages.h")
with open(STAGES) as _f:
    _TEXT = _f.read()
KIND = {k: i + 1 for i, k in enumerate(re.findall(r"\bK_\w+", re.search(r"enum Kind : uint32_t \{(.*?)\}", _TEXT, re.S).group(1)))}
WIDTHS = (4, 5, 6, 16)
CLASS_COUNTS = {}


def count(cls, n=1):
    CLASS_COUNTS[cls] = CLASS_COUNTS.get(cls, 0) + n


# ---- scalars ---------------------------------------------------------------------------------------------------------------
def positions(w):
    return {4: 64, 16: 16}.get(w, (252 + w) // w)


def digits(s, w):
    """The digits the product must act on, computed the textbook way (not by adding a constant): signed digits in
    [-2^(w-1), 2^(w-1)) from the bottom and an unsigned top digit that takes the rest; plain 16-bit digits for the comb."""
    if w == 16:
        return [(s >> (16 * i)) & 0xFFFF for i in range(16)]
    out = []
    for _ in range(positions(w) - 1):
        d = s & ((1 << w) - 1)
        if d >= 1 << (w - 1):
            d -= 1 << w
        out.append(d)
        s = (s - d) >> w
    return out + [s]


def from_digits(ds, w):
    return sum(d << (w * i) for i, d in enumerate(ds))


def recode_constant(w):
    """what recode_signed4 / kt_recode add: 2^(w-1) at every position but the top one"""
    return sum(1 << (w * i + w - 1) for i in range(positions(w) - 1))


def scalars(w, prng, n_random=300):
    """[(class, scalar)] for window width w, all below r"""
    n = positions(w)
    lo, hi = (0, 0xFFFF) if w == 16 else (-(1 << (w - 1)), (1 << (w - 1)) - 1)
    shift = w * (n - 1)
    out = [("small", s) for s in (0, 1, 2, 7, 8, 9, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2)]
    ks = sorted({k + d for k in range(252) if k % w == 0 or k % 32 == 0 for d in (-1, 0, 1) if 0 <= k + d <= 251})
    out += [("pow2", 1 << k) for k in ks] + [("pow2_minus_1", (1 << k) - 1) for k in ks]

    def with_top(cls, low):
        """the digits `low` below the smallest and below the largest top digit that keep the scalar in [0, r)"""
        base = from_digits(low, w)
        tmin, tmax = max(0, -(base >> shift)), (R - 1 - base) >> shift
        return [(cls, base + (t << shift)) for t in sorted({tmin, tmax}) if tmin <= t <= tmax]

    out += with_top("digits_most_positive", [hi] * (n - 1)) + with_top("digits_most_negative", [lo] * (n - 1))
    out += with_top("digits_alternating", ([hi, lo] * n)[:n - 1]) + with_top("digits_alternating", ([lo, hi] * n)[:n - 1])
    top_max = digits(R - 1, w)[-1]
    for p in range(n):
        for d in ((1, hi) if p < n - 1 else (1, top_max)):
            if d << (w * p) < R:              # the top window alone reaches r for w = 4 and 6: out_of_range_scalars has those
                out.append(("one_digit_top_window" if p == n - 1 else "one_digit", d << (w * p)))
        if p < n - 1 and lo < 0:
            out.append(("one_negative_digit", (1 << (w * (p + 1))) + (lo << (w * p))))     # digit p = lo under a 1
    out += [("largest_top_digit", R - 1)] + [("largest_top_digit", s) for s in (top_max << shift,) if s < R]
    if w != 16:
        c = recode_constant(w)
        for j in range(1, 8):
            m = 1 << (32 * j)
            low = (m - c % m) % m                            # s + c carries out of the low j words, which come out zero
            for high in (0, prng.randrange(R >> (32 * j))):
                out += [("carry_through_words" if j == 7 else "carry_chain", (high << (32 * j)) + low),
                        ("carry_chain", (high << (32 * j)) + low - 1)]
        out.append(("carry_chain_250_bits", (1 << 250) - c % (1 << 250)))
    out += [("random", prng.randrange(R)) for _ in range(n_random)]
    seen, uniq = set(), []
    for cls, s in out:
        assert 0 <= s < R, (w, cls, s)
        count("w%d %s" % (w, cls))
        if s not in seen:
            seen.add(s)
            uniq.append((cls, s))
    # the generator's own claims, checked with the textbook digits
    d_all = {cls: [digits(s, w) for c2, s in out if c2 == cls] for cls in {c for c, _ in out}}
    assert any(all(x == hi for x in d[:-1]) for d in d_all["digits_most_positive"]), w
    assert any(all(x == lo for x in d[:-1]) for d in d_all["digits_most_negative"]), w
    every = [d for ds in d_all.values() for d in ds]
    for p in range(n - 1):
        assert any(d[p] != 0 and sum(1 for x in d if x) == 1 for d in every), (w, p)
        assert any(d[p] == hi for d in every) and any(d[p] == lo for d in every), (w, p)
    assert max(d[-1] for d in every) == top_max
    return uniq


def out_of_range_scalars(w):
    """Scalars of 256 bits, which only a malformed item carries (status 3 whatever is computed): the look-up must stay inside
    its table.  [(scalar, the multiple the clamp makes of it)]: a top digit beyond the table's last entry counts as that entry."""
    last = 8 if w == 4 else (1 << (w - 1))
    shift = w * (positions(w) - 1)
    out = []
    # the top window alone (one non-zero digit there), which is below r only for w = 5; then 256-bit patterns.  All of them
    # leave s + recode_constant(w) below 2^256: beyond that the sum wraps and the digits mean nothing (memory safety alone
    # matters there, and the clamp that gives it is exercised here).
    for s in (1 << shift, digits(R - 1, w)[-1] << shift, (1 << 256) - (1 << 253), 9 << 252, (15 << 252) + 12345, R, R + 1, 1 << 255):
        assert s + recode_constant(w) < 1 << 256
        top = digits(s, w)[-1]
        count("w%d one_digit_top_window" % w, int(s == top << shift))
        out.append((s, s - ((top - last) << shift) if top > last else s))
        count("w%d out_of_range" % w)
        count("w%d out_of_range_clamped" % w, int(top > last))
    return out


# ---- points ----------------------------------------------------------------------------------------------------------------
def point_classes(prng):
    t8 = torsion_generator()
    tors = [o.mul(t8, k) for k in range(1, 8)]
    p1, p2 = o.mul(o.G, prng.randrange(1, R)), o.mul(o.G_NUMS, prng.randrange(1, R))
    pts = [("G", o.G), ("G_nums", o.G_NUMS), ("prime_order", p1), ("prime_order", p2), ("negated", o.neg(p1)),
           ("identity", o.IDENTITY)]
    pts += [("torsion", t) for t in tors] + [("prime_plus_torsion", o.add(p1, t)) for t in tors]
    assert o.mul(t8, 8) == o.IDENTITY and len({o.IDENTITY, *tors}) == 8 and all(o.is_on_curve(p) for _, p in pts)
    for cls, _ in pts:
        count("point " + cls)
    return pts


# ---- records ---------------------------------------------------------------------------------------------------------------
def w8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def pt16(p):
    return w8(p[0]) + w8(p[1])


def record(name, kind, param, rows, meta):
    assert len(rows) == len(meta) and rows
    return {"name": name, "kind": kind, "code": KIND[kind] << 24 | param, "param": param, "rows": rows, "meta": meta}


def mul_items(sc_list, pts, prng, special_every=9):
    """(point, scalar) pairs: every scalar on G and on a random prime-order point; the special points (negated, identity,
    torsion, prime + torsion) on every `special_every`-th scalar and on the small ones.  Shuffled, so that the lanes of a
    wave take different digits."""
    items = []
    special = [(c, p) for c, p in pts if c not in ("G", "G_nums", "prime_order")]
    for i, (cls, s) in enumerate(sc_list):
        items.append((o.G, s))
        items.append((pts[2][1], s))
        if cls == "small" or i % special_every == 0:
            items += [(p, s) for _, p in special[i % 3::3]]
    prng.shuffle(items)
    return items


def eq_row(mode, u, c, pk, r, gen):
    return w8(u) + w8(c) + pt16(pk) + pt16(r) + pt16(gen) + [mode, 0, 0, 0]


def equation_items(prng, sc4, sc16):
    """Items of both equations.  meta: (mode, u, c, PK, R, Gen, prime) with prime = every point is of prime order"""
    from test_hostbuild import half_size_cases
    from helpers import to_int
    items = []
    t8 = torsion_generator()
    g2 = o.mul(o.G, prng.randrange(1, R))

    def add(cls, mode, u, c, pk, gen, r=None, prime=True):
        base = (o.G, o.G_NUMS, gen)[mode]
        good = o.add(o.mul(base, u), o.mul(pk, c))
        for rr in ((good, o.add(good, o.G)) if r is None else (r,)):
            items.append((mode, u, c, pk, rr, gen, prime))
            count("eq %s %s" % (("fixed", "fixed", "per_item_gen")[mode], cls))

    # per-item generator: the crafted scalars on u (table 1) and on c (table 0), the other one ordinary
    for i, (cls, s) in enumerate(sc4):
        if cls == "random" and i % 6:
            continue
        sk = prng.randrange(1, R)
        pk = o.mul(g2, sk)
        if i % 2:
            add("crafted_u", 2, s, prng.randrange(1 << 250), pk, g2)
        else:
            add("crafted_c", 2, prng.randrange(R), s, pk, g2)
    # degenerate relations inside one item: the Straus loop adds a point to itself and to its negative
    for s in (1, 2, 7, 8, 0x0777 << 236, R - 1, prng.randrange(R)):
        rnd = prng.randrange(R)
        add("pk_is_gen_equal_scalars", 2, s, s, g2, g2)
        add("pk_is_minus_gen_equal_scalars", 2, s, s, o.neg(g2), g2)
        add("gen_is_g", 2, s, rnd, o.mul(o.G, 5), o.G)
        add("pk_is_g", 0, s, rnd % (1 << 250), o.G, o.G)
        add("pk_is_minus_g", 0, s, rnd % (1 << 250), o.neg(o.G), o.G)
        pk = o.mul(o.G, rnd or 1)
        add("pk_is_r", 0, s, rnd % (1 << 250), pk, o.G, r=pk)
        add("pk_is_minus_r", 1, s, rnd % (1 << 250), pk, o.G, r=o.neg(pk))
        add("pk_is_r", 2, s, rnd, o.mul(g2, 3), g2, r=o.mul(g2, 3))
    # fixed generator: the adversarial Euclid inputs as challenges (a, |b| at their extremes, both signs of b), u crafted
    c_arr, n_special = half_size_cases()
    cs = [to_int(c_arr[i]) for i in range(n_special + 40)]
    us = [s for cls, s in sc16 if cls != "random"]
    for i, c in enumerate(cs):
        sk = (1, R - 1, prng.randrange(1, R))[i % 3] if i % 4 == 0 else prng.randrange(1, R)
        mode = i & 1
        pk = o.mul((o.G, o.G_NUMS)[mode], sk)
        add("euclid_challenge", mode, us[i % len(us)], c, pk, o.G)
        if i % 3 == 0:
            add("u_is_zero", mode, 0, c, pk, o.G)              # b*u = 0 (mod r): no negation of zero
    for i, u in enumerate(us):
        mode = i & 1
        add("crafted_u", mode, u, prng.randrange(1 << 250), o.mul((o.G, o.G_NUMS)[mode], prng.randrange(1, R)), o.G)
    # points with torsion: the verdict is the half-size sum's, evaluated by the oracle
    for k in range(1, 8):
        sk, u, c = prng.randrange(1, R), prng.randrange(R), prng.randrange(1 << 250)
        pk = o.mul(o.G, sk)
        r = o.add(o.mul(o.G, u), o.mul(pk, c))
        tk, tj = o.mul(t8, k), o.mul(t8, (3 * k) % 8)
        add("torsion", 0, u, c, o.add(pk, tk), o.G, r=r, prime=False)
        add("torsion", 0, u, c, pk, o.G, r=o.add(r, tk), prime=False)
        add("torsion", 0, u, c, o.add(pk, tk), o.G, r=o.add(r, tj), prime=False)
        add("torsion", 2, u, c, o.add(pk, tk), o.G, r=o.add(r, o.mul(tk, c)), prime=False)
    prng.shuffle(items)
    return items


def build_records(device=False):
    """every record of one run: [record], in the order they are written"""
    CLASS_COUNTS.clear()
    prng = random.Random(0x5CA1A8)
    sc = {w: scalars(w, prng) for w in WIDTHS}
    pts = point_classes(prng)
    recs = []
    comb = [(which, s) for _, s in sc[16] for which in (0, 1)]
    prng.shuffle(comb)
    recs.append(record("comb_mul", "K_COMB", 0, [w8(s) + [which, 0, 0, 0] for which, s in comb], comb))
    tab = [(p, s, s) for p, s in mul_items(sc[4], pts, prng)] + [(pts[2][1], s, eff) for s, eff in out_of_range_scalars(4)]
    recs.append(record("table_mul", "K_TABLE", 0, [pt16(p) + w8(s) for p, s, _ in tab], tab))
    eqs = equation_items(prng, sc[4], sc[16])
    rows = [eq_row(*m[:6]) for m in eqs]
    recs.append(record("check_equation", "K_EQ", 0, rows, eqs))
    for w in (5, 6):
        kt = [(p, s, s) for p, s in mul_items(sc[w], pts, prng, 13)] + [(pts[3][1], s, eff) for s, eff in out_of_range_scalars(w)]
        recs.append(record("kt_add_scalar w=%d" % w, "K_KT", w, [pt16(p) + w8(s) for p, s, _ in kt], kt))
        one_per_class = list({c: p for c, p in pts}.items())
        recs.append(record("kt tables w=%d" % w, "K_KT_DUMP", w, [pt16(p) + [0] * 8 for _, p in one_per_class], one_per_class))
        if device:
            recs.append(record("kt bases quad w=%d" % w, "K_KT_BASES_QUAD", w, recs[-1]["rows"], one_per_class))
    for pos in (4, 8, 16):
        recs.append(record("sb pieces positions=%d" % pos, "K_SB", pos, rows, eqs))
        some = eqs[:23]
        recs.append(record("sb tables positions=%d" % pos, "K_SB_TABLES", pos, rows[:23], some))
        if device:
            recs.append(record("sb tables quad positions=%d" % pos, "K_SB_TABLES_QUAD", pos, rows[:23], some))
    for cls in ("eq fixed euclid_challenge", "eq fixed u_is_zero", "eq fixed torsion", "eq per_item_gen torsion",
                "eq per_item_gen pk_is_gen_equal_scalars", "eq per_item_gen pk_is_minus_gen_equal_scalars", "eq fixed pk_is_g",
                "eq fixed pk_is_minus_g", "eq fixed pk_is_r", "eq fixed pk_is_minus_r", "eq per_item_gen pk_is_r",
                "eq per_item_gen gen_is_g", "eq per_item_gen crafted_u", "eq per_item_gen crafted_c", "eq fixed crafted_u"):
        assert CLASS_COUNTS.get(cls, 0) > 0, cls
    for w in WIDTHS:
        for cls in ("small", "pow2", "pow2_minus_1", "digits_most_positive", "digits_most_negative", "digits_alternating",
                    "one_digit", "one_digit_top_window", "largest_top_digit", "random") + \
                (("one_negative_digit", "carry_chain", "carry_through_words", "carry_chain_250_bits", "out_of_range") if w != 16 else ()):
            assert CLASS_COUNTS.get("w%d %s" % (w, cls), 0) > 0, (w, cls)
    assert CLASS_COUNTS["w4 out_of_range_clamped"] > 0 and CLASS_COUNTS["w5 out_of_range_clamped"] > 0
    for cls in ("G", "G_nums", "prime_order", "negated", "identity", "torsion", "prime_plus_torsion"):
        assert CLASS_COUNTS.get("point " + cls, 0) > 0, cls
    assert sum(1 for r in recs if len(r["rows"]) % 64) * 2 > len(recs)        # most records end in a partly filled wave
    return recs


OUT_WORDS = {"K_COMB": lambda p: 36, "K_TABLE": lambda p: 36, "K_EQ": lambda p: 18, "K_KT": lambda p: 38,
             "K_KT_DUMP": lambda w: positions(w) * 36 * (2 + (1 << (w - 1))), "K_KT_BASES_QUAD": lambda w: positions(w) * 36,
             "K_SB": lambda p: 46, "K_SB_TABLES": lambda p: 2 * p * 324, "K_SB_TABLES_QUAD": lambda p: 2 * p * 324}


def input_words(recs):
    return np.concatenate([np.array([r["code"], len(r["rows"])] + sum(r["rows"], []), np.uint32) for r in recs])


def output_words(recs):
    return sum(len(r["rows"]) * OUT_WORDS[r["kind"]](r["param"]) for r in recs)


def attach_outputs(recs, out):
    """cut the output words into records; prints each record with its case count"""
    pos = 0
    for r in recs:
        n, w = len(r["rows"]), OUT_WORDS[r["kind"]](r["param"])
        r["out"] = out[pos:pos + n * w].reshape(n, w)
        pos += n * w
        print("%-32s %5d cases%s" % (r["name"], n, "" if n % 64 == 0 else ", last wave partly filled"))
    assert pos == len(out)
    for cls in sorted(CLASS_COUNTS):
        print("  class %-52s %5d" % (cls, CLASS_COUNTS[cls]))
    return {r["name"]: r for r in recs}


# ---- checks ----------------------------------------------------------------------------------------------------------------
def plain(l):
    return limbs_val(l) * RINV % Q


def check_fe(l, what, units=2):
    assert all(int(x) < 1 << 29 for x in l[:8]) and limbs_val(l) < units * Q, what


def check_point(out, want, what, t_valid=True):
    """as test_device_edges_gpu.check_point, with the bounds of ext_pt's coordinates (fe_n: normalised limbs, below 2q)"""
    for j in range(4):
        check_fe(out[9 * j:9 * j + 9], what)
    X, Y, Z, T = (plain(out[9 * j:9 * j + 9]) for j in range(4))
    u, v = want
    assert Z != 0 and X == u * Z % Q and Y == v * Z % Q, what
    if t_valid:
        assert T * Z % Q == X * Y % Q, what


def check_niels(e, want, what):
    """a cached addend (Y+X, Y-X, Z, 2dT) of the point `want`: fe_t coordinates (normalised limbs, below 5q)"""
    for j in range(4):
        check_fe(e[9 * j:9 * j + 9], what, 5)
    ypx, ymx, z, t2d = (plain(e[9 * j:9 * j + 9]) for j in range(4))
    u, v = want
    assert z != 0 and ypx == (v + u) * z % Q and ymx == (v - u) * z % Q and t2d == D2 * u * v % Q * z % Q, what


_MUL = {}


def mul(p, k):
    key = (p, k)
    if key not in _MUL:
        _MUL[key] = o.mul(p, k % R) if k >= 1 << 256 else o.mul(p, k)
    return _MUL[key]


def check_comb(recs):
    r = recs["comb_mul"]
    for (which, s), out in zip(r["meta"], r["out"]):
        check_point(out, mul((o.G, o.G_NUMS)[which], s), ("comb", which, hex(s)), t_valid=False)


def check_table(recs):
    r = recs["table_mul"]
    for (p, s, eff), out in zip(r["meta"], r["out"]):
        check_point(out, mul(p, eff), ("table_mul", p, hex(s)))


def check_kt(recs):
    for w in (5, 6):
        r = recs["kt_add_scalar w=%d" % w]
        for (p, s, eff), out in zip(r["meta"], r["out"]):
            check_point(out[:36], mul(p, eff), ("kt_add_scalar", w, p, hex(s)))
            valid = o.point_is_valid(p)
            assert (int(out[36]), int(out[37])) == (2 if valid else 0, int(valid)), (w, p)
        d = recs["kt tables w=%d" % w]
        n, entries = positions(w), (1 << (w - 1)) + 1
        for (cls, p), out in zip(d["meta"], d["out"]):
            base = p
            for i in range(n):
                if i:
                    base = mul(base, 1 << w)
                check_point(out[36 * i:36 * i + 36], base, ("kt base", w, cls, i))
                tab = out[36 * n + 36 * entries * i:]
                acc = o.IDENTITY
                for j in range(entries):
                    check_niels(tab[36 * j:36 * j + 36], acc, ("kt table", w, cls, i, j))
                    acc = o.add(acc, base)
        q = recs.get("kt bases quad w=%d" % w)
        if q is not None:
            assert (q["out"] == d["out"][:, :36 * n]).all(), w                 # bit for bit


def half_size_verdict(m, out):
    """What a fixed-generator item must give: (a, b) checked against the textbook Euclid, then (b*u)G + a*PK - b*R == O
    evaluated by the oracle; for points of prime order that is u*G + c*PK == R, which is checked too."""
    from test_hostbuild import check_half_size
    mode, u, c, pk, r, gen, prime = m
    a = sum(int(x) << (32 * i) for i, x in enumerate(out[1:5]))
    b = sum(int(x) << (32 * i) for i, x in enumerate(out[5:9]))
    check_half_size([fe_bytes(c)], [a.to_bytes(16, "little")], [b.to_bytes(16, "little")], [int(out[0])])
    sb = -b if out[0] else b
    base = (o.G, o.G_NUMS)[mode]
    total = o.add(o.add(mul(base, sb * u % R), mul(pk, a)), o.neg(mul(r, b)) if sb > 0 else mul(r, b))
    want = total == o.IDENTITY
    if prime:
        assert want == (o.add(mul(base, u), mul(pk, c)) == r), m
    return want, sb, total


def check_equations(recs):
    r = recs["check_equation"]
    held = 0
    for m, out in zip(r["meta"], r["out"]):
        mode, u, c, pk, rr, gen, prime = m
        if mode < 2:
            want, sb, _ = half_size_verdict(m, out[1:10])
            assert sum(int(x) << (32 * i) for i, x in enumerate(out[10:18])) == sb * u % R, m
            count("half_size b negative" if sb < 0 else "half_size b positive")
        else:
            want = o.add(mul(gen, u), mul(pk, c)) == rr
        assert int(out[0]) == int(want), m
        held += int(want)
    assert 0 < held < len(r["meta"])
    assert CLASS_COUNTS.get("half_size b negative", 0) > 0 and CLASS_COUNTS.get("half_size b positive", 0) > 0


def check_latency_path(recs):
    for pos in (4, 8, 16):
        r = recs["sb pieces positions=%d" % pos]
        for m, out in zip(r["meta"], r["out"]):
            mode, u, c, pk, rr, gen, prime = m
            if mode < 2:
                want, _, total = half_size_verdict(m, out[1:10])
            else:
                total = o.add(mul(gen, u), mul(pk, c))
                want = total == rr
            assert int(out[0]) == int(want), (pos, m)
            check_point(out[10:46], total, (pos, m))
        t = recs["sb tables positions=%d" % pos]
        for m, out in zip(t["meta"], t["out"]):
            mode, u, c, pk, rr, gen, prime = m
            windows = 32 if mode < 2 else 64
            for pt, p in enumerate((pk, rr if mode < 2 else gen)):
                for k in range(pos):
                    base = mul(p, 1 << (4 * (windows // pos) * k))
                    acc = o.IDENTITY
                    for j in range(9):
                        e = out[324 * (pt * pos + k) + 36 * j:][:36]
                        check_niels(e, acc, ("sb table", pos, pt, k, j, m))
                        acc = o.add(acc, base)
        q = recs.get("sb tables quad positions=%d" % pos)
        if q is not None:
            assert (q["out"] == t["out"]).all(), pos                          # bit for bit


# ---- the comb tables, every entry ----------------------------------------------------------------------------------------
def limbs_to_ints(l):
    """(n, 9) normalised limbs (the first eight below 2^29) -> n Python integers, packed with numpy"""
    l = np.ascontiguousarray(l, dtype=np.uint64)
    words = np.zeros((len(l), 5), np.uint64)
    for i in range(9):
        word, sh = divmod(29 * i, 64)
        words[:, word] |= l[:, i] << np.uint64(sh)
        if sh + (32 if i == 8 else 29) > 64:
            words[:, word + 1] |= l[:, i] >> np.uint64(64 - sh)
    raw = words.tobytes()
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") for i in range(len(l))]


def comb_row_reference(base, i, bits):
    """b * 2^(bits i) * base for every b, as (n, 64) affine bytes: the C oracle's point addition (held against o.add and o.mul
    on a sample by the caller), doubling the list bits times"""
    import jjs_oracle_c as oc
    step = o.mul(base, 1 << (bits * i))
    pts = np.stack([pt_bytes(o.IDENTITY)])
    for k in range(bits):
        pts = np.concatenate([pts, oc.point_add(pts, np.tile(pt_bytes(o.mul(step, 1 << k)), (len(pts), 1)))])
    return pts, step


def check_comb_table(tab, base, sample_rng):
    """tab (windows, entries, 28) uint32: every entry is (y+x, y-x, 2dxy) of b * 2^(bits i) * base in Montgomery form, within
    the bounds add_comb_range assumes when it loads the words as fe_t (normalised limbs, value below 5q); padding word 0."""
    windows, entries = tab.shape[0], tab.shape[1]
    bits = entries.bit_length() - 1
    assert tab.shape[2] == 28 and not tab[:, :, 27].any()
    limbs = tab[:, :, :27].reshape(windows, entries, 3, 9)
    assert (limbs[..., :8] < (1 << 29)).all()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(1) as pool:                    # the next row's additions (C, outside the interpreter lock) beside this row's comparison
        nxt = pool.submit(comb_row_reference, base, 0, bits)
        for i in range(windows):
            ref, step = nxt.result()
            if i + 1 < windows:
                nxt = pool.submit(comb_row_reference, base, i + 1, bits)
            for b in [0, 1, 2, entries - 1] + [int(x) for x in sample_rng.integers(0, entries, 6)]:     # the C oracle against the Python one
                want = o.mul(step, b)
                assert ref[b].tobytes() == pt_bytes(want).tobytes(), (i, b)
                if 0 < b:
                    assert ref[b].tobytes() == pt_bytes(o.add(o.mul(step, b - 1), step)).tobytes(), (i, b)
            raw = ref.tobytes()
            vals = limbs_to_ints(limbs[i].reshape(-1, 9))
            assert max(vals) < 5 * Q, i
            xs = [int.from_bytes(raw[64 * b:64 * b + 32], "little") for b in range(entries)]
            ys = [int.from_bytes(raw[64 * b + 32:64 * b + 64], "little") for b in range(entries)]
            want = [w for x, y in zip(xs, ys) for w in ((y + x) % Q, (y - x) % Q, D2 * x * y % Q)]
            got = [v * RINV % Q for v in vals]
            if got != want:
                bad = next(k for k in range(len(got)) if got[k] != want[k])
                raise AssertionError("comb entry (row %d, b %d, coordinate %d) is not that multiple of the base" % (i, bad // 3, bad % 3))


# ---- degenerate relations inside one item, as valid signatures (through the ABI) ----------------------------------------------
def degenerate_batch(scheme, seed=0xDE6E):
    """Items signed with the oracle's arithmetic whose points coincide: PK = G (sk = 1), PK = -G (sk = r - 1), PK = R and
    PK = -R (nonce = +-sk); for the per-item generator also Gen = G and PK = Gen.  Every other one has its message changed
    afterwards (status 2).  A batch dict like helpers.make_batch; the expected statuses come from helpers.oracle_verify."""
    from helpers import ARG_ORDER, fe_arr, pt_arr
    prng = random.Random(seed)
    rows = {k: [] for k in ARG_ORDER[scheme]}
    rnd = lambda: prng.randrange(1, R)  # noqa: E731
    plans = [("pk_is_g", 1, rnd(), None), ("pk_is_minus_g", R - 1, rnd(), None)]
    for _ in range(2):
        sk = rnd()
        plans += [("pk_is_r", sk, sk, None), ("pk_is_minus_r", sk, R - sk, None), ("ordinary", sk, rnd(), None)]
    if scheme == "vargen":
        plans += [("gen_is_g", rnd(), rnd(), 1), ("gen_is_g_pk_is_gen", 1, rnd(), 1), ("pk_is_gen_is_r", 1, 1, rnd())]
    for i, (cls, sk, k, g) in enumerate(plans * 2):
        gen = o.mul(o.G, g if g is not None else rnd()) if scheme == "vargen" else o.G
        pk, r, m = o.mul(gen, sk), o.mul(gen, k), prng.randrange(Q)
        vals = {"R": r, "PK": pk}
        if scheme == "single":
            c = o.challenge_single(r, pk, m)
        elif scheme == "double":
            vals.update(Rp=o.mul(o.G_NUMS, k), PKp=o.mul(o.G_NUMS, sk))
            c = o.challenge_double(r, vals["Rp"], pk, vals["PKp"], m)
        else:
            vals["Gen"] = gen
            c = o.challenge_vargen(r, pk, gen, m)
        if cls == "pk_is_r":
            assert pk == r
        if cls == "pk_is_minus_r":
            assert pk == o.neg(r)
        rows["u"].append((k - c * sk) % R)
        rows["m"].append(m ^ 1 if i >= len(plans) and i % 2 else m)
        for name, p in vals.items():
            rows[name].append(p)
        count("abi %s %s" % (scheme, cls))
    return {k: (fe_arr(v) if k in ("u", "m") else pt_arr(v)) for k, v in rows.items()}

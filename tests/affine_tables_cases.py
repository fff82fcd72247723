"""Inputs and checks for the affine key tables (csrc/key_tables.h: kt_build_table leaves (v+u, v-u, 1, 2d u v), kt_add_digit adds
with the 7-product formula, kt_add_challenge skips the position a 250-bit scalar leaves empty), shared by the CPU build
(test_affine_tables_host.py) and the device (test_affine_tables_gpu.py).  Records of tools/scalar_stages.h; every output is
compared with the Python oracle's big-integer curve arithmetic through the checks of scalar_mul_cases.py."""
import random

import jjs_oracle as o
import scalar_mul_cases as smc
from helpers import const_table

Q, R = o.Q, o.R_ORDER
ONE = [int(x) for x in const_table("JJS_ONE")]          # the Montgomery form of one, canonical limbs
assert smc.limbs_val(ONE) == (1 << 261) % Q


def crafted_items(w, pts, prng):
    """(point, scalar, the multiple it must give): every crafted scalar of scalar_mul_cases.scalars (24 random ones) on G or on
    a random prime-order point in turn, every 11th also on the special points; then the 256-bit scalars of a malformed item."""
    special = [p for c, p in pts if c not in ("G", "G_nums", "prime_order")]
    items = []
    for i, (cls, s) in enumerate(smc.scalars(w, prng, n_random=24)):
        items.append(((o.G, pts[2][1])[i % 2], s, s))
        if cls == "small" or i % 11 == 0:
            items += [(p, s, s) for p in special[i % 3::3]]
    prng.shuffle(items)
    return items + [(pts[3][1], s, eff) for s, eff in smc.out_of_range_scalars(w)]


def challenges(w, prng, n):
    """n challenges below 2^250 for window width w, the crafted ones first"""
    top = (1 << 250) - 1
    if w == 6:
        low = lambda pick: sum(pick() << (6 * i) for i in range(41))  # noqa: E731  raw 6-bit digits of positions 0 .. 40
        cs = [0, 1, top, (15 << 246) + low(lambda: 63), (15 << 246) + low(lambda: 32), (15 << 246) + low(lambda: prng.randrange(32, 64)),
              1 << 249, (1 << 246) - 1, 1 << 246]
        for c in cs[3:6]:
            assert c >> 246 == 15 and all((c >> (6 * i)) & 63 >= 32 for i in range(41))
    else:
        cs = [0, 1, top, 1 << 249, (1 << 249) - 1, top - smc.recode_constant(5) % (1 << 250)]
        assert smc.digits(top, 5)[-1] == 1 and smc.digits(1 << 249, 5)[-1] == 1 and smc.digits(1, 5)[-1] == 0
    cs += [prng.randrange(1 << 250) for _ in range(n - len(cs))]
    for c in cs:
        d = smc.digits(c, w)
        assert 0 <= c < 1 << 250 and smc.from_digits(d, w) == c
        if w == 6:
            assert d[-1] == 0 and 0 <= d[-2] <= 17, hex(c)      # the dead position, and the bound on the one below it
    if w == 6:
        assert max(smc.digits(c, 6)[-2] for c in cs) >= 16
    return cs


def build_records():
    """[record] in the order they are written.  The challenge record of the wide windows is one full wave of 64 items; the
    others end in a partly filled wave."""
    prng = random.Random(0xAFF1E)
    pts = smc.point_classes(prng)
    every = [p for _, p in pts]
    recs = []
    for w in (5, 6):
        one_per_class = list({c: p for c, p in pts}.items())
        recs.append(smc.record("kt tables w=%d" % w, "K_KT_DUMP", w, [smc.pt16(p) + [0] * 8 for _, p in one_per_class], one_per_class))
        kt = crafted_items(w, pts, prng)
        recs.append(smc.record("kt_add_scalar w=%d" % w, "K_KT", w, [smc.pt16(p) + smc.w8(s) for p, s, _ in kt], kt))
        n = 64 if w == 6 else 37
        ch = [(every[i % len(every)] if i % 3 == 2 else (o.G, pts[2][1])[i % 2], c) for i, c in enumerate(challenges(w, prng, n))]
        recs.append(smc.record("kt_add_challenge w=%d" % w, "K_KT_CHALLENGE", w, [smc.pt16(p) + smc.w8(c) for p, c in ch], ch))
    assert len(recs[-1]["rows"]) == 64 and sum(1 for r in recs if len(r["rows"]) % 64) >= 4
    return recs


OUT_WORDS = dict(smc.OUT_WORDS, K_KT_CHALLENGE=lambda w: 36)


def output_words(recs):
    return sum(len(r["rows"]) * OUT_WORDS[r["kind"]](r["param"]) for r in recs)


def attach_outputs(recs, out):
    pos = 0
    for r in recs:
        n, w = len(r["rows"]), OUT_WORDS[r["kind"]](r["param"])
        r["out"] = out[pos:pos + n * w].reshape(n, w)
        pos += n * w
        print("%-28s %5d cases" % (r["name"], n))
    assert pos == len(out)
    return {r["name"]: r for r in recs}


def check_tables_are_affine(recs):
    """every entry j >= 1: the z slot is one EXACTLY, every limb of every coordinate is below 2^29, and the entry is j * base by
    the oracle (check_niels: (v+u) z, (v-u) z, 2d u v z with the z it finds); entry 0 is the identity's (1, 1, 1, 0)"""
    for w in (5, 6):
        d = recs["kt tables w=%d" % w]
        n, entries = smc.positions(w), (1 << (w - 1)) + 1
        for (cls, p), out in zip(d["meta"], d["out"]):
            base = p
            for i in range(n):
                if i:
                    base = smc.mul(base, 1 << w)
                smc.check_point(out[36 * i:36 * i + 36], base, ("kt base", w, cls, i))
                tab = out[36 * n + 36 * entries * i:][:36 * entries]
                assert int(tab.max()) < 1 << 29, (w, cls, i)
                acc = o.IDENTITY
                for j in range(entries):
                    e = tab[36 * j:36 * j + 36]
                    assert [int(x) for x in e[18:27]] == ONE, (w, cls, i, j)
                    smc.check_niels(e, acc, ("kt table", w, cls, i, j))
                    acc = o.add(acc, base)
                assert [int(x) for x in tab[:18]] == ONE + ONE and not tab[27:36].any(), (w, cls, i)


def check_scalars(recs):
    for w in (5, 6):
        r = recs["kt_add_scalar w=%d" % w]
        for (p, s, eff), out in zip(r["meta"], r["out"]):
            smc.check_point(out[:36], smc.mul(p, eff), ("kt_add_scalar", w, p, hex(s)))
            valid = o.point_is_valid(p)
            assert (int(out[36]), int(out[37])) == (2 if valid else 0, int(valid)), (w, p)


def check_challenges(recs):
    for w in (5, 6):
        r = recs["kt_add_challenge w=%d" % w]
        for (p, c), out in zip(r["meta"], r["out"]):
            smc.check_point(out, smc.mul(p, c), ("kt_add_challenge", w, p, hex(c)))

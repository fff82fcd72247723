"""Inputs and checks of the ingest tests, shared by the CPU build (test_ingest_host.py) and the device (test_ingest_gpu.py):
crafted inputs for the inversion by division steps (csrc/fq_inv.h), the inverse square root and the point decoding
(csrc/decode.h), the shared inversion of extended coordinates (csrc/normalize.h) and the square-root tables; the records of
tools/ingest_stages.h; and the comparison of every output word with Python integers -- pow(x, q - 2, q), the 2-adic logarithm
found bit by bit, oracle.decompress, U / Z -- never with the host build and never with the device.  Every class of case is
counted; CLASS_COUNTS is asserted non-zero class by class, so a change here cannot silently empty one.

The division steps have a model here (inverse_model), written from the definition in Bernstein and Yang's paper: it says how
many steps an input needs, with which sign f ends, and which of the final corrections an input takes."""
import functools
import os
import random
import re

import numpy as np

import jjs_oracle as o
from helpers import limbs_val, torsion_generator, wire_point_cases

Q = o.Q
T_ODD = (Q - 1) >> 32                       # q - 1 = 2^32 t
ZETA = pow(7, T_ODD, Q)                     # generator of the 2^32-torsion (7 is a non-residue)
ZETA_INV = pow(ZETA, -1, Q)
T_INV = pow(T_ODD, -1, 1 << 32)
G8 = pow(ZETA, 1 << 24, Q)                  # order 256
RP = 1 << 261                               # the Montgomery radix of csrc/fq29.h
RP_INV = pow(RP, -1, Q)
assert pow(ZETA, 1 << 31, Q) == Q - 1 and pow(G8, 128, Q) == Q - 1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "ingest_stages.h")) as _f:
    _TEXT = _f.read()
KIND = {k: i + 1 for i, k in enumerate(re.findall(r"\bK_\w+", re.search(r"enum Kind : uint32_t \{(.*?)\}", _TEXT, re.S).group(1)))}
NORM_FILL = int(re.search(r"NORM_FILL = (0x[0-9A-Fa-f]+)u", _TEXT).group(1), 16)
NORM_FILL_BYTE = int(re.search(r"NORM_FILL_BYTE = (0x[0-9A-Fa-f]+)u", _TEXT).group(1), 16)
with open(os.path.join(ROOT, "jubjub_schnorr_amd", "csrc", "jjs_constants.inc")) as _f:
    _CONST = _f.read()
HASH_MULT = int(re.search(r"#define JJS_DLOG_HASH_MULT (\w+?)u?\s", _CONST).group(1), 0)
HASH_SHIFT = int(re.search(r"#define JJS_DLOG_HASH_SHIFT (\d+)", _CONST).group(1))
CLASS_COUNTS = {}


def count(cls, n=1):
    CLASS_COUNTS[cls] = CLASS_COUNTS.get(cls, 0) + n


def w8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_w8(row):
    return sum(int(x) << (32 * i) for i, x in enumerate(row))


# ---- the division steps, from the paper's definition -----------------------------------------------------------------------
#   divstep(delta, f, g) = (1 - delta, g, (g - f) / 2)               if delta > 0 and g is odd
#                          (1 + delta, f, (g + (g mod 2) f) / 2)     otherwise
# started at delta = 1/2 (the half-step variant), f = q, g = a.  D below is 2 delta.
def divstep_count(a):
    """the number of division steps after which g = 0"""
    D, f, g, n = 1, Q, a, 0
    while g:
        if D > 0 and g & 1:
            D, f, g = 2 - D, g, (g - f) >> 1
        else:
            D, g = D + 2, (g + (g & 1) * f) >> 1
        n += 1
    return n


QINV30 = pow(Q, -1, 1 << 30)


def inverse_model(a, batches=20):
    """1 / a by `batches` batches of 30 division steps, with Python integers.  A batch is collected into the integer matrix
    2^30 (f', g') = ((u, v), (q, r)) (f, g) and applied to (d, e), which start at (0, 1), modulo q: d' = (u d + v e + m q) / 2^30
    with the one m that makes the division exact in (s - 2^30, s], where s adds u for a negative d and v for a negative e (the
    arrangement that keeps d and e in (-2q, q)).  At the end g = 0, f = +-1 and d = +-1/a: q is added if d is negative, the sign
    of f is applied, and q is added once more if the value is negative then.
    Returns the inverse and what the input did: steps, sign of f, d negative before the end, first and second addition."""
    D, f, g, d, e, steps = 1, Q, a, 0, 1, 0
    for _ in range(batches):
        u, v, q, r = 1, 0, 0, 1
        for _ in range(30):
            steps += g != 0
            if D > 0 and g & 1:
                D, f, g = 2 - D, g, (g - f) >> 1
                u, v, q, r = 2 * q, 2 * r, q - u, r - v
            else:
                b = g & 1
                D, g = D + 2, (g + b * f) >> 1
                u, v, q, r = 2 * u, 2 * v, q + b * u, r + b * v
        nd, ne = u * d + v * e, q * d + r * e
        sd, se = (u if d < 0 else 0) + (v if e < 0 else 0), (q if d < 0 else 0) + (r if e < 0 else 0)
        md, me = sd - ((QINV30 * nd + sd) & 0x3FFFFFFF), se - ((QINV30 * ne + se) & 0x3FFFFFFF)
        nd, ne = nd + md * Q, ne + me * Q
        assert nd & 0x3FFFFFFF == 0 and ne & 0x3FFFFFFF == 0
        d, e = nd >> 30, ne >> 30
        assert -2 * Q < d < Q and -2 * Q < e < Q
    info = {"steps": steps, "finished": g == 0, "f": f, "d_negative": d < 0}
    x = d + Q if d < 0 else d
    x = -x if f < 0 else x
    info["second_addition"] = x < 0
    x = x + Q if x < 0 else x
    return x, info


@functools.lru_cache(maxsize=None)
def long_step_search(n_random=3000, n_climb=1500, seed=0x57E9):
    """A bounded, seeded search for inputs with many division steps: random values, then single-bit changes of the best that
    are kept when they do not shorten the count.  (values with their counts, the counts of the random part)"""
    prng = random.Random(seed)
    pool = [(divstep_count(a), a) for a in (prng.randrange(1, Q) for _ in range(n_random))]
    spread = [c for c, _ in pool]
    best = sorted(pool, reverse=True)[:8]
    for i in range(n_climb):
        c, a = best[i % len(best)]
        b = (a ^ (1 << prng.randrange(255))) % Q
        if b:
            cb = divstep_count(b)
            if cb >= c and (cb, b) not in best:
                best[i % len(best)] = (cb, b)
    return sorted(set(best), reverse=True), spread


HOSTBUILD_SPECIALS = [0, 1, 2, 3, Q - 1, Q - 2, (Q + 1) // 2, (Q - 1) // 2, 2**254, 2**254 + 1, 2**255 - 19 - Q] + \
    [2**k for k in (29, 30, 31, 32, 58, 59, 60, 64, 87, 90, 120, 232, 240, 253)] + [2**k - 1 for k in (29, 30, 60, 90, 240, 254)] + \
    [Q - 2**k for k in (1, 29, 30, 60, 200)] + [pow(3, k, Q) for k in (100, 1000, 10**6)]     # the list of test_hostbuild.py


@functools.lru_cache(maxsize=None)
def inversion_cases(n_random=2000):
    """[(class, value)], all below q, and STEP_STATS"""
    prng = random.Random(0x1A7)
    out = [("hostbuild special", v % Q) for v in HOSTBUILD_SPECIALS]
    for bits in (30, 60, 90):                                  # whole batches of pure halvings
        out += [("low %d bits zero" % bits, x) for x in (1 << bits, 3 << bits, ((Q >> bits) - 1) << bits, (prng.randrange(Q >> bits) | 1) << bits,
                                                         prng.randrange(1, Q >> bits) << bits)]
    for bits in (29, 30):                                      # limb patterns of both radices, kept below 2^254 < q
        for i in range(9):
            for cls, pat in (("all ones", (1 << bits) - 1), ("lowest bit", 1), ("highest bit", 1 << (bits - 1))):
                v = (pat << (bits * i)) & ((1 << 254) - 1)
                if v:
                    out.append(("%d-bit limb %s" % (bits, cls), v))
        out.append(("%d-bit limbs alternating all ones" % bits, sum(((1 << bits) - 1) << (bits * i) for i in range(0, 9, 2)) & ((1 << 254) - 1)))
        out.append(("%d-bit limbs alternating all ones" % bits, sum(((1 << bits) - 1) << (bits * i) for i in range(1, 9, 2)) & ((1 << 254) - 1)))
    for k in range(255):
        out += [("q - 2^k", Q - (1 << k)), ("q + 2^k", (Q + (1 << k)) % Q)]
        if k >= 1:
            out += [("(q +- 1) / 2^k", (Q - 1) >> k), ("(q +- 1) / 2^k", (Q + 1) >> k)]     # the same value from k = 2 on
    found, spread = long_step_search()
    out += [("longest step counts found", a) for _, a in found]
    out += [("random", prng.randrange(Q)) for _ in range(n_random)]
    seen, uniq = set(), []
    for cls, v in out:
        assert 0 <= v < Q, (cls, v)
        if v not in seen:
            seen.add(v)
            uniq.append((cls, v))
            count("inv " + cls)
    # what the model says each input does: the classes of the end of the algorithm
    steps = []
    for _, v in uniq:
        x, info = inverse_model(v)
        assert info["finished"] and x == (pow(v, Q - 2, Q) if v else 0), hex(v)
        if v:
            assert abs(info["f"]) == 1
            steps.append(info["steps"])
            count("inv model: f = +1" if info["f"] > 0 else "inv model: f = -1")
            count("inv model: d not negative before the end", int(not info["d_negative"]))
            count("inv model: second addition of q", int(info["second_addition"]))
            count("inv model: no addition of q", int(not info["d_negative"] and not info["second_addition"]))
            # A batch that starts with g = 0 is u = 2^30, v = 0: it adds q to a negative d and leaves any other d alone.  Two
            # of them lift every d of (-2q, q) into [0, q), so an input that is done within 18 batches cannot leave d negative,
            # and no input found needs more (STEP_STATS).  normalize_30's first addition is met through K_FINISH instead.
            assert info["steps"] > 540 or not info["d_negative"], hex(v)
            count(NEGATIVE_D, int(info["d_negative"]))
    STEP_STATS.update(min=min(steps), max=max(steps), mean=sum(steps) / len(steps), random_max=max(spread), random_min=min(spread),
                      search_max=found[0][0], over_570=sum(1 for s in steps if s > 570))
    return uniq


STEP_STATS = {}
# The figures that DESIGN.md 6.8 and the docstrings of the two test modules quote.  The tests hold what a run finds against them,
# so a change of a seed or of a case list has to change the record too; they are a record, not a bound on the step count.
RECORDED = {"steps_min": 501, "steps_max": 531, "steps_mean": 514, "random_min": 500, "random_max": 527, "search_max": 531,
            "inversion_cases": 2816, "inv_sqrt_cases": 2318, "decompress_cases": 2126, "valid_drawn": 1391, "update_cases": 2560}


def check_recorded():
    inversion_cases(), decompress_cases()
    found = {"steps_min": STEP_STATS["min"], "steps_max": STEP_STATS["max"], "steps_mean": round(STEP_STATS["mean"]),
             "random_min": STEP_STATS["random_min"], "random_max": STEP_STATS["random_max"], "search_max": STEP_STATS["search_max"],
             "inversion_cases": len(inversion_cases()), "inv_sqrt_cases": len(inv_sqrt_cases()),
             "decompress_cases": len(decompress_cases()[0]), "valid_drawn": DRAWS["valid"], "update_cases": len(update_cases())}
    assert found == RECORDED, (found, RECORDED)
NEGATIVE_D = "inv model: d negative before the end (first addition of q)"      # the one class that may stay empty: see above


def s30_limbs(x):
    """nine limbs of 30 bits, the top one signed, as uint32 words"""
    return [(x >> (30 * i)) & 0x3FFFFFFF for i in range(8)] + [(x >> 240) & 0xFFFFFFFF]


@functools.lru_cache(maxsize=None)
def finish_cases():
    """[(class, d, sign word)] for normalize_30 alone: d over the whole of (-2q, q), both signs of f"""
    prng = random.Random(0xF1)
    ds = [("d in (-2q, -q)", d) for d in [-2 * Q + 1, -Q - 1] + [-Q - prng.randrange(1, Q) for _ in range(24)]]
    ds += [("d in [-q, 0)", d) for d in [-Q, -Q + 1, -1, -(1 << 240), -(1 << 30)] + [-prng.randrange(1, Q) for _ in range(24)]]
    ds += [("d in [0, q)", d) for d in [0, 1, Q - 1, 1 << 240, (1 << 240) - 1] + [prng.randrange(Q) for _ in range(24)]]
    out = []
    for cls, d in ds:
        for sign in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF, 0x80000000):
            out.append((cls, d, sign))
            x = d + Q if d < 0 else d
            x = -x if sign >> 31 else x
            count("finish " + cls)
            count("finish first addition of q", int(d < 0))
            count("finish second addition of q", int(x < 0))
            count("finish both additions of q", int(d < 0 and x < 0))
            count("finish f negative" if sign >> 31 else "finish f positive")
    return out


def update_expected(d, e, u, v, q, r):
    """one batch applied to (d, e) modulo q, as inverse_model does it: the one multiple of q that makes the division by 2^30
    exact in (s - 2^30, s], where s adds a row's first entry for a negative d and its second for a negative e"""
    out = []
    for a, b in ((u, v), (q, r)):
        n = a * d + b * e
        s = (a if d < 0 else 0) + (b if e < 0 else 0)
        m = s - ((QINV30 * n + s) & 0x3FFFFFFF)
        assert (n + m * Q) & 0x3FFFFFFF == 0
        x = (n + m * Q) >> 30
        assert -2 * Q < x < Q and (x << 30) % Q == n % Q
        out.append(x)
    return out


def real_batches(a):
    """[(d, e, u, v, q, r)] before each batch of inverse_model(a)"""
    D, f, g, d, e, out = 1, Q, a, 0, 1, []
    for _ in range(20):
        u, v, q, r = 1, 0, 0, 1
        for _ in range(30):
            if D > 0 and g & 1:
                D, f, g = 2 - D, g, (g - f) >> 1
                u, v, q, r = 2 * q, 2 * r, q - u, r - v
            else:
                b = g & 1
                D, g = D + 2, (g + b * f) >> 1
                u, v, q, r = 2 * u, 2 * v, q + b * u, r + b * v
        out.append((d, e, u, v, q, r))
        d, e = update_expected(d, e, u, v, q, r)
    return out


@functools.lru_cache(maxsize=None)
def update_cases():
    """[(class, d, e, u, v, q, r)] for update_de_30 alone"""
    prng = random.Random(0xDE30)
    edge = [-2 * Q + 1, -2 * Q + 2, -Q - 1, -Q, -Q + 1, -1, 0, 1, Q - 2, Q - 1]
    H = 1 << 30
    rows = [(H, 0), (-H, 0), (0, H), (0, -H), (H // 2, H // 2), (-H // 2, -H // 2), (H // 2, -H // 2), (-H // 2, H // 2), (H - 1, 1), (1, 1 - H),
            (1, 0), (0, 1), (0, 0), (-1, -1)]
    for _ in range(6):                                           # |a| + |b| = 2^30 with random split and signs
        a = prng.randrange(1, H)
        rows.append((a * prng.choice((1, -1)), (H - a) * prng.choice((1, -1))))
    out = []
    for i, (u, v) in enumerate(rows):
        q, r = rows[(i + 7) % len(rows)]
        for d in edge:
            for e in edge:
                out.append(("edge operands", d, e, u, v, q, r))
        for _ in range(8):
            d, e = (prng.randrange(-2 * Q + 1, Q) for _ in range(2))
            out.append(("random operands", d, e, u, v, q, r))
    for a in (1, 2, Q - 1, (Q + 1) // 2, long_step_search()[0][0][1]) + tuple(prng.randrange(1, Q) for _ in range(15)):
        out += [("batches of a real inversion",) + t for t in real_batches(a)]
    for cls, d, e, u, v, q, r in out:
        assert abs(u) + abs(v) <= H and abs(q) + abs(r) <= H and -2 * Q < d < Q and -2 * Q < e < Q
        count("update " + cls)
        count("update |u| + |v| = 2^30", int(abs(u) + abs(v) == H))
        count("update d and e negative", int(d < 0 and e < 0))
        count("update d negative alone", int(d < 0 <= e))
        count("update e negative alone", int(e < 0 <= d))
        count("update neither negative", int(d >= 0 and e >= 0))
    return out


def check_update(cases, out):
    assert len(out) == len(cases)
    for (cls, d, e, u, v, q, r), row in zip(cases, out):
        d2, e2 = update_expected(d, e, u, v, q, r)
        assert [int(w) for w in row] == s30_limbs(d2) + s30_limbs(e2) + [0, 0], (cls, d, e, u, v, q, r)


def check_finish(cases, out):
    assert len(out) == len(cases)
    for (cls, d, sign), row in zip(cases, out):
        x = d + Q if d < 0 else d
        x = -x if sign >> 31 else x
        x = x + Q if x < 0 else x
        assert 0 <= x < Q
        assert [int(w) for w in row] == s30_limbs(x) + [0], (cls, d, hex(sign))


# ---- the 2-adic logarithm and the inverse square root ----------------------------------------------------------------------
ZINV_POW2 = [pow(ZETA_INV, 1 << i, Q) for i in range(32)]


def dlog32(b):
    """k with zeta^k == b, for b in the 2^32-torsion: one bit at a time from the bottom"""
    k = 0
    for i in range(32):
        if pow(b, 1 << (31 - i), Q) != 1:
            k |= 1 << i
            b = b * ZINV_POW2[i] % Q
    assert b == 1
    return k


def inv_sqrt_expected(y):
    """what fq_inv_sqrt documents: w * zeta^(-(k >> 1)) with w = y^((t-1)/2) and zeta^k = y^t; 0 for 0.  (value, k)"""
    if y == 0:
        return 0, None
    w = pow(y, (T_ODD - 1) // 2, Q)
    k = dlog32(y * w * w % Q)
    return w * pow(ZETA_INV, k >> 1, Q) % Q, k


def with_log(k, x):
    """y = zeta^m x^(2^32) with m = k / t mod 2^32: y^t = zeta^k"""
    return pow(ZETA, k * T_INV % (1 << 32), Q) * pow(x, 1 << 32, Q) % Q


@functools.lru_cache(maxsize=None)
def inv_sqrt_cases():
    """[(class, y, k or None)]"""
    prng = random.Random(0x5A27)
    ks = []
    for pos in range(4):
        for val in range(256):
            if pos == 0 and val & 1:
                continue                                         # the odd low bytes: the non-squares below
            k = (prng.getrandbits(32) & ~(0xFF << (8 * pos)) | val << (8 * pos)) & ~1
            ks.append(("byte %d takes every value" % pos, k))
    ks += [("all bytes 0", 0), ("all bytes 255 (not a square)", 0xFFFFFFFF), ("all bytes 254", 0xFEFEFEFE), ("k = 2^31", 1 << 31),
           ("k = 2^32 - 2", (1 << 32) - 2)]
    ks += [("odd low byte (not a square)", (prng.getrandbits(24) << 8) | k0) for k0 in range(1, 256, 2)]
    out = []
    for cls, k in ks:
        for xcls, x in (("pure torsion", 1), ("times a random 2^32-th power", prng.randrange(1, Q))):
            y = with_log(k, x)
            assert pow(y, T_ODD, Q) == pow(ZETA, k, Q)
            assert (pow(y, (Q - 1) // 2, Q) == 1) == (k % 2 == 0)
            out.append((cls, y, k))
            count("sqrt " + cls)
            count("sqrt " + xcls)
    out += [("zero", 0, None), ("one", 1, 0), ("q - 1", Q - 1, 1 << 31), ("zeta", ZETA, T_ODD % (1 << 32))]
    out += [("g8^j", pow(G8, j, Q), (j << 24) * T_ODD % (1 << 32)) for j in range(256)]
    for cls, _, _ in out[-260:]:
        count("sqrt " + cls)
    for pos in range(4):                                         # the generator's claim, on the k of all cases
        want = set(range(0, 256, 2)) if pos == 0 else set(range(256))
        assert want <= {(k >> (8 * pos)) & 0xFF for _, _, k in out if k is not None and k % 2 == 0}, pos
    assert {k & 0xFF for _, _, k in out if k is not None and k & 1} == set(range(1, 256, 2))
    return out


def check_inv_sqrt(cases, out):
    assert len(out) == len(cases)
    for (cls, y, k), row in zip(cases, out):
        got = from_w8(row)
        want, k2 = inv_sqrt_expected(y)
        assert k2 == k, (cls, hex(y))
        assert got == want, (cls, hex(y), k)
        if k is not None and k % 2 == 0:
            assert got * got * y % Q == 1, (cls, hex(y))


def check_inv(cases, out):
    assert len(out) == len(cases)
    for (cls, x), row in zip(cases, out):
        assert from_w8(row) == (pow(x, Q - 2, Q) if x else 0), (cls, hex(x))


# ---- compressed points -----------------------------------------------------------------------------------------------------
def log_of_v(v):
    """the logarithm k that decoding v meets: of y^t with y = (v^2 - 1)(1 + d v^2); None for y = 0"""
    v2 = v * v % Q
    y = (v2 - 1) * (1 + o.D * v2) % Q
    return dlog32(pow(y, T_ODD, Q)) if y else None


def enc_of(v, sign):
    return (v | sign << 255).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def decompress_cases():
    """[(class, 32 bytes)] and the oracle's answers [point or None]"""
    prng = random.Random(0xDEC0)
    out = [("wire_point_cases", e) for e in wire_point_cases(np.random.default_rng(31))]
    vs = [0, 1, 2, Q - 2, Q - 1, Q, Q + 1, (1 << 255) - 1] + [1 << (29 * i) for i in range(9)] + [(1 << (32 * i)) - 1 for i in range(1, 9)]
    out += [("chosen v, both signs", enc_of(v & ((1 << 255) - 1), s)) for v in vs for s in (0, 1)]
    t8 = torsion_generator()
    out += [("torsion point", o.compress(o.mul(t8, k))) for k in range(8)]
    out += [("v = 0: u^2 = -1", enc_of(0, s)) for s in (0, 1)]
    assert all(o.decompress(e)[0] ** 2 % Q == Q - 1 for _, e in out[-2:])
    out += [("u = 0 with the sign bit", enc_of(1, 1)), ("u = 0 with the sign bit", enc_of(Q - 1, 1))]
    # valid encodings until the logarithm has taken every byte value at every position
    need = {(p, b) for p in range(4) for b in range(256) if p or b % 2 == 0}
    kept = draws = 0
    while need:
        draws += 1
        assert draws < 8192
        v = prng.randrange(Q)
        k = log_of_v(v)
        if k is None or k & 1:
            continue
        need -= {(p, (k >> (8 * p)) & 0xFF) for p in range(4)}
        out.append(("random valid, every byte of k", enc_of(v, prng.getrandbits(1))))
        kept += 1
    DRAWS["valid"], DRAWS["drawn"] = kept, draws
    need, v = set(range(1, 256, 2)), 1
    while need:
        v += 1
        k = log_of_v(v)
        if k is not None and k & 1:
            need.discard(k & 0xFF)
            out.append(("small v without a root, every odd k0", enc_of(v, v & 1)))
    DRAWS["no_root_up_to"] = v
    want = [o.decompress(e) for _, e in out]
    for (cls, e), w in zip(out, want):
        count("dec " + cls)
        count("dec accepted" if w is not None else "dec rejected")
        if w is not None:
            assert o.compress(w) == e
    return out, want


DRAWS = {}


def decompress_expected_bytes(want):
    """(n, 64) affine bytes and (n,) ok: (0, 1) and 0 where the oracle rejects"""
    aff = np.frombuffer(b"".join(o.le32(w[0]) + o.le32(w[1]) if w is not None else o.le32(0) + o.le32(1) for w in want), np.uint8)
    return aff.reshape(-1, 64).copy(), np.array([w is not None for w in want], np.uint8)


def check_decompress(cases, want, aff, ok):
    """aff (n, 64) and ok (n,) against the oracle; the accepted ones compressed back give their input"""
    want_aff, want_ok = decompress_expected_bytes(want)
    assert aff.shape == want_aff.shape and len(ok) == len(want_ok)
    for i, (cls, e) in enumerate(cases):
        assert int(ok[i]) == int(want_ok[i]), (i, cls, e.hex())
        assert aff[i].tobytes() == want_aff[i].tobytes(), (i, cls, e.hex())
        if want_ok[i]:
            back = bytearray(aff[i, 32:].tobytes())
            back[31] |= (int(aff[i, 0]) & 1) << 7
            assert bytes(back) == e, (i, cls)


# ---- extended coordinates --------------------------------------------------------------------------------------------------
def norm_record(name, n_src, n, lanes, first=0, after=0, edits=(), prng=None):
    """A K_NORMALIZE record: rows = first + n + after rows of random (u z, v z, z); `edits` is [(source, item, {U/V/Z: value})]
    with `item` counted from `first`."""
    rows = first + n + after
    pts = [[[0, 0, 0] for _ in range(rows)] for _ in range(n_src)]
    for k in range(n_src):
        for i in range(rows):
            u, v, z = prng.randrange(Q), prng.randrange(Q), prng.randrange(1, Q)
            pts[k][i] = [u * z % Q, v * z % Q, z]
    for k, item, change in edits:
        for c, val in change.items():
            pts[k][first + item]["UVZ".index(c)] = val
    return {"name": name, "kind": "K_NORMALIZE", "code": KIND["K_NORMALIZE"] << 24 | n_src, "count": rows, "n_src": n_src, "n": n,
            "first": first, "lanes": lanes, "rows": rows, "pts": pts,
            "payload": [n, first, lanes, 0] + [w for k in range(n_src) for i in range(rows) for c in range(3) for w in w8(pts[k][i][c])]}


@functools.lru_cache(maxsize=None)
def normalize_records():
    prng = random.Random(0x4042)
    big = (1 << 256) - 1
    recs = []
    n = 37
    for n_src in (1, 2, 3, 4):
        for j, lanes in enumerate((1, 2, 64, n, n + 3, 5)):       # 5 does not divide 37
            first, after = ((0, 0), (3, 2), (16, 5))[(j + n_src) % 3]
            edits = [(prng.randrange(n_src), prng.randrange(n), {"Z": 0}), (prng.randrange(n_src), prng.randrange(n), {"Z": 1})]
            recs.append(norm_record("n_src=%d lanes=%d first=%d" % (n_src, lanes, first), n_src, n, lanes, first, after, edits, prng))
            count("norm lanes %s" % {1: "1", 2: "2", 64: "64", n: "n", n + 3: "n + 3", 5: "no divisor of n"}[lanes])
            count("norm n_src %d" % n_src)
            count("norm first > 0, rows before and after", int(first > 0 and after > 0))
    recs.append(norm_record("one lane owns 300 items", 2, 300, 1, 2, 1, [(0, 150, {"Z": 0})], prng))
    recs.append(norm_record("two lanes own 300 items each", 3, 600, 2, 0, 0, [(1, 599, {"Z": 0}), (2, 0, {"Z": 1})], prng))
    count("norm a lane of 300 items", 2)
    # lanes = 4, 40 items: lane 1 owns 1, 5, .., 37 -- Z = 0 at its first, a middle and its last item; every Z of lane 2 is zero
    edits = [(0, 1, {"Z": 0}), (1, 17, {"Z": 0}), (0, 37, {"Z": 0})] + [(k, i, {"Z": 0}) for k in (0, 1) for i in range(2, 40, 4)]
    count("norm Z = 0 at the first, a middle and the last item of a lane", 3)
    count("norm a lane whose Z are all zero")
    # lane 0 (items 0, 4, ..): the values of Z, U and V at and beyond q
    edits += [(0, 0, {"Z": 1}), (1, 4, {"Z": Q - 1}), (0, 8, {"Z": Q}), (1, 12, {"Z": Q + 1}), (0, 16, {"Z": big}),
              (0, 20, {"U": 0}), (1, 20, {"V": 0}), (0, 24, {"U": Q}), (1, 28, {"V": Q}), (0, 32, {"U": big}), (1, 36, {"V": big}),
              (1, 3, {"U": Q, "Z": 0}), (0, 7, {"V": big, "Z": Q})]
    count("norm Z in {1, q - 1, q, q + 1, 2^256 - 1}", 5)
    count("norm U or V in {0, q, 2^256 - 1}", 6)
    count("norm malformed together with Z = 0 or Z = q", 2)
    recs.append(norm_record("zero and non-canonical coordinates", 2, 40, 4, 5, 3, edits, prng))
    # all 16 zero masks of a four-point item, on 3 lanes, twice (so that every lane meets several)
    edits = [(k, i, {"Z": 0}) for i in range(32) for k in range(4) if (i % 16) >> k & 1]
    recs.append(norm_record("the 16 zero masks of a four-point item", 4, 35, 3, 1, 1, edits, prng))
    count("norm zero masks of a four-point item", 16)
    return recs


def normalize_expected(r):
    """(affine words per source: rows x 16, bytes per row) of a K_NORMALIZE record, with Python integers"""
    rows, first, n = r["rows"], r["first"], r["n"]
    aff = np.full((r["n_src"], rows, 16), NORM_FILL, np.uint32)
    bad = np.full(4 * ((rows + 3) // 4), NORM_FILL_BYTE, np.uint8)
    for i in range(first, first + n):
        bad[i] = int(any(c >= Q for k in range(r["n_src"]) for c in r["pts"][k][i]))
        for k in range(r["n_src"]):
            U, V, Z = r["pts"][k][i]
            zi = pow(1 if (Z == 0 or Z >= Q) else Z, Q - 2, Q)       # a Z that is zero or not canonical counts as 1
            u, v = (0, 0) if Z == 0 else (U % Q * zi % Q, V % Q * zi % Q)
            aff[k, i] = w8(u) + w8(v)
    return aff, bad


def check_normalize(r):
    aff, bad = normalize_expected(r)
    got_aff = r["out"][:aff.size].reshape(aff.shape)
    got_bad = r["out"][aff.size:].view(np.uint8)
    for k in range(r["n_src"]):
        for i in range(r["rows"]):
            assert got_aff[k, i].tolist() == aff[k, i].tolist(), (r["name"], "source", k, "row", i, [hex(c) for c in r["pts"][k][i]])
    assert got_bad.tolist() == bad.tolist(), (r["name"], np.nonzero(got_bad != bad)[0][:8])


# ---- the square-root tables ------------------------------------------------------------------------------------------------
def tables_expected_values():
    """pow[i][j] as plain values: zeta^(-j 2^(8i)) for i < 3, zeta^(-(j >> 1)) for i = 3, zeta^(-j 2^(8(i-3)-1)) beyond"""
    out = np.empty((7, 256), object)
    for i in range(7):
        for j in range(256):
            e = j << (8 * i) if i < 3 else (j >> 1 if i == 3 else j << (8 * (i - 3) - 1))
            out[i, j] = pow(ZETA_INV, e, Q)
    return out


def hash_keys():
    """the slot of g8^j: ((limb 0 of the canonical Montgomery form) * MULT >> SHIFT) & 0xffff, from the generated constants"""
    return [((((pow(G8, j, Q) * RP % Q) & 0x1FFFFFFF) * HASH_MULT & 0xFFFFFFFF) >> HASH_SHIFT) & 0xFFFF for j in range(256)]


def check_tables(pw, hs, same_as=None):
    """pw (7, 256, 9) uint32, hs (65536,) uint8; same_as: the (pw, hs) of the CPU build of the same source, bit for bit"""
    pw, hs = np.asarray(pw).reshape(7, 256, 9), np.asarray(hs).reshape(65536)
    want = tables_expected_values()
    for i in range(7):
        for j in range(256):
            l = [int(x) for x in pw[i, j]]
            assert all(x < 1 << 29 for x in l) and limbs_val(l) < 2 * Q, (i, j)
            assert limbs_val(l) * RP_INV % Q == want[i, j], (i, j)
    keys = hash_keys()
    assert len(set(keys)) == 256
    for j, key in enumerate(keys):
        assert int(hs[key]) == j, (j, key)
    rest = np.ones(65536, bool)
    rest[keys] = False
    assert not hs[rest].any()
    if same_as is not None:
        assert np.array_equal(pw, np.asarray(same_as[0]).reshape(7, 256, 9)), np.argwhere(pw != np.asarray(same_as[0]).reshape(7, 256, 9))[:4]
        assert np.array_equal(hs, np.asarray(same_as[1]).reshape(65536))


# ---- records ---------------------------------------------------------------------------------------------------------------
OUT_WORDS = {"K_INV": 8, "K_INV_SQRT": 8, "K_DECOMPRESS": 20, "K_FINISH": 10, "K_UPDATE": 20}


def item_record(name, kind, rows):
    return {"name": name, "kind": kind, "code": KIND[kind] << 24, "count": len(rows), "payload": [w for row in rows for w in row]}


def build_records():
    dec, _ = decompress_cases()
    recs = [item_record("inverse", "K_INV", [w8(x) for _, x in inversion_cases()]),
            item_record("inverse square root", "K_INV_SQRT", [w8(y) for _, y, _ in inv_sqrt_cases()]),
            item_record("decompress", "K_DECOMPRESS", [w8(int.from_bytes(e, "little")) for _, e in dec])]
    recs.append(item_record("end of the inversion", "K_FINISH", [s30_limbs(d) + [sign, 0, 0] for _, d, sign in finish_cases()]))
    recs.append(item_record("one batch applied to d and e", "K_UPDATE",
                            [s30_limbs(d) + s30_limbs(e) + [x & 0xFFFFFFFF for x in (u, v, q, r)] + [0, 0] for _, d, e, u, v, q, r in update_cases()]))
    recs += [dict(r) for r in normalize_records()]
    recs.append({"name": "tables", "kind": "K_TABLES", "code": KIND["K_TABLES"] << 24, "count": 1, "payload": []})
    return recs


def record_out_words(r):
    if r["kind"] == "K_NORMALIZE":
        return r["n_src"] * r["rows"] * 16 + (r["rows"] + 3) // 4
    if r["kind"] == "K_TABLES":
        return 7 * 256 * 9 + 65536 // 4
    return r["count"] * OUT_WORDS[r["kind"]]


def input_words(recs):
    return np.concatenate([np.array([r["code"], r["count"]] + r["payload"], np.uint32) for r in recs])


def output_words(recs):
    return sum(record_out_words(r) for r in recs)


def attach_outputs(recs, out):
    """cut the output words into records; prints each record with its case count"""
    pos = 0
    for r in recs:
        w = record_out_words(r)
        r["out"] = out[pos:pos + w]
        pos += w
        print("%-48s %5d %s" % (r["name"], r["count"], "rows" if r["kind"] == "K_NORMALIZE" else "cases"))
    assert pos == len(out)
    for cls in sorted(CLASS_COUNTS):
        print("  class %-64s %5d" % (cls, CLASS_COUNTS[cls]))
    print("  division steps:", STEP_STATS, " draws:", DRAWS)
    return {r["name"]: r for r in recs}


def table_dump(r):
    """(pow, hash) of a K_TABLES record's output"""
    return r["out"][:7 * 256 * 9].reshape(7, 256, 9), r["out"][7 * 256 * 9:].view(np.uint8)

"""Inputs and checks of the tests of the arithmetic modulo the group order r, shared by the CPU build (test_fr_host.py) and the
device (test_fr_gpu.py): the records of tools/fr_stages.h -- fr_mont_mul, fr_mul, fr_sub_mul, fr_add, half_scalar_times_u,
truncate250, chacha20_block and bv_weights -- and the comparison of every output word with Python integers (`%`, `pow`) and
with a ChaCha20 written here from RFC 8439 section 2.3, never with the CPU build and never with the device.  mont_model is a
model of fr_mont_mul's loop; it only CLASSIFIES inputs (which take the final subtraction, which reach the words t[8] / t[9]),
it is never the expectation.  Every class of case is counted; CLASS_COUNTS is asserted non-zero class by class, so a change
here cannot silently empty one.  The one exemption is EXEMPT_CLASSES (DESIGN.md 6.10 gives the reason)."""
import functools
import json
import os
import random
import re

import numpy as np

import jjs_oracle as o

Q, R = o.Q, o.R_ORDER
M32, M256 = (1 << 32) - 1, (1 << 256) - 1
R_INV256 = pow(1 << 256, -1, R)
FR_INV32 = (-pow(R, -1, 1 << 32)) % (1 << 32)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STAGES = os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "fr_stages.h")
with open(STAGES) as _f:
    _TEXT = _f.read()
KIND = {k: i + 1 for i, k in enumerate(re.findall(r"\bK_\w+", re.search(r"enum Kind : uint32_t \{(.*?)\}", _TEXT, re.S).group(1)))}
# (words in, words out) per kind, as the stages of tools/fr_stages.h declare them
SHAPE = {"K_MONT_MUL": (16, 8), "K_MUL": (16, 8), "K_SUB_MUL": (24, 8), "K_ADD": (16, 8), "K_HALF_TIMES_U": (16, 8),
         "K_TRUNCATE250": (12, 10), "K_CHACHA20": (12, 16), "K_WEIGHTS": (12, 16)}
WEIGHT_BITS = (129, 131, 134, 135, 139, 143)           # msm_weight_bits(c) for the window widths 8 .. 16 of the device
PINNED_SEED = bytes(range(32))                         # batch_seed() under jjs_debug_pin_hash_seed(2)
WEIGHT_ITEMS = (0, 1, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) + 5, 1 << 40)
N_RANDOM = 2000
CLASS_COUNTS = {}
# a pre-subtraction value of exactly r needs a b + m r = r 2^256 with m < 2^256, so r | a b, so a = 0 or b = 0 for canonical
# inputs (r is prime), and then m = 0 and the value is 0: the class cannot occur
EXEMPT_CLASSES = ("mont_mul canonical: pre-subtraction value equal to r",)
OUT_OF_CONTRACT_GE_R = {}                              # recorded by check_mont_mul, not asserted


def count(cls, n=1):
    CLASS_COUNTS[cls] = CLASS_COUNTS.get(cls, 0) + n


# ---- ChaCha20, RFC 8439 section 2.3 ----------------------------------------------------------------------------------------
def _rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


def _quarter(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & M32; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & M32; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & M32; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & M32; s[b] = _rotl(s[b] ^ s[c], 7)


def chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    """The block function: 32-byte key, 32-bit counter, 12-byte nonce -> 64 bytes of keystream."""
    assert len(key) == 32 and len(nonce) == 12 and 0 <= counter <= M32
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)] + \
        [counter] + [int.from_bytes(nonce[4 * i:4 * i + 4], "little") for i in range(3)]
    s = list(init)
    for _ in range(10):
        _quarter(s, 0, 4, 8, 12); _quarter(s, 1, 5, 9, 13); _quarter(s, 2, 6, 10, 14); _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15); _quarter(s, 1, 6, 11, 12); _quarter(s, 2, 7, 8, 13); _quarter(s, 3, 4, 9, 14)
    return b"".join(((x + y) & M32).to_bytes(4, "little") for x, y in zip(s, init))


def check_chacha20_against_rfc():
    v = json.load(open(os.path.join(HERE, "golden", "chacha20_rfc8439.json")))
    assert chacha20_block(bytes.fromhex(v["key"]), v["counter"], bytes.fromhex(v["nonce"])).hex() == v["block"]
    return v


def weights(seed: bytes, item: int, bits: int):
    """(z, z') of item `item`: block `item` of the keystream (counter = low word, nonce word 0 = high word), bytes 0-19 and
    20-39 as little-endian integers, cut to `bits` bits"""
    blk = chacha20_block(seed, item & M32, (item >> 32).to_bytes(4, "little") + bytes(8))
    mask = (1 << bits) - 1
    return int.from_bytes(blk[:20], "little") & mask, int.from_bytes(blk[20:40], "little") & mask


# ---- the model of fr_mont_mul's loop (classification only) -----------------------------------------------------------------
def mont_model(a, b):
    """-> (value of t[0..8] before the subtraction, subtraction taken, t[9] after a row of products or t[8] after a row's
    reduction was non-zero at some step)"""
    t, high = 0, False
    for i in range(8):
        t += a * ((b >> (32 * i)) & M32)
        high = high or (t >> 288) != 0
        mq = ((t & M32) * FR_INV32) & M32
        t = (t + mq * R) >> 32
        high = high or (t >> 256) != 0
    return t, not ((t >> 256) == 0 and (t & M256) < R), high


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def canonical_edges():
    k0 = ((1 << 252) - R + (1 << 32) - 1) >> 32                 # the smallest k with 2^252 - 2^32 k < r
    e = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 250) - 1, 1 << 251, (1 << 252) - (k0 << 32), (1 << 252) - ((k0 + 1) << 32)]
    e += [1 << (32 * i) for i in range(1, 8)] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
    assert all(0 <= x < R for x in e) and len(set(e)) == len(e)
    assert (1 << 252) - ((k0 - 1) << 32) >= R
    return e


OUT_OF_CONTRACT = (R, R + 1, (1 << 252) - 1, 1 << 255, (1 << 256) - 1)


def product_pairs(prng, fn):
    """[(class, a, b)] for fr_mont_mul (fn = "mont_mul") or fr_mul (fn = "mul"), all canonical"""
    e = canonical_edges()
    out = [("canonical edges", a, b) for a in e for b in e]
    for bits in WEIGHT_BITS:
        ws = [(1 << bits) - 1, 1 << (bits - 1)] + [prng.randrange(1 << bits) for _ in range(10)]
        cs = [(1 << 250) - 1, 0, 1] + [prng.randrange(1 << 250) for _ in range(5)]
        us = [R - 1, R - 2] + [prng.randrange(R) for _ in range(5)]
        out += [("weight-shaped %d bits x c" % bits, w, c) for w in ws for c in cs]
        out += [("weight-shaped %d bits x u" % bits, w, u) for w in ws for u in us]
    # the final conditional subtraction: a seeded search over random pairs for those the model says take it.  (For fr_mul
    # the product that decides is the second one, of a 2^256 mod r with b.)
    first = (lambda a: a) if fn == "mont_mul" else (lambda a: a * (1 << 256) % R)
    taken, tries = 0, 0
    while taken < 320:
        a, b = prng.randrange(R), prng.randrange(R)
        tries += 1
        assert tries < 400000
        if mont_model(first(a), b)[1]:
            out.append(("final subtraction taken (random search)", a, b))
            taken += 1
    # ... and pairs whose result is a chosen target next to 0 or next to r - 1: b = target 2^256 / a' for a random a'
    for side in ("0", "r - 1"):
        n = 0
        while n < (2400 if side == "0" else 320):
            a = prng.randrange(1, R)
            d = prng.choice((0, 1, 2, 3, prng.randrange(1 << 16), prng.randrange(1 << 32)))
            target = d if side == "0" else R - 1 - d
            b = target * pow(first(a) * R_INV256 % R, -1, R) % R
            out.append(("result next to " + side, a, b))
            n += 1
    out += [("random", prng.randrange(R), prng.randrange(R)) for _ in range(N_RANDOM)]
    for cls, a, b in out:
        assert 0 <= a < R and 0 <= b < R
        count("%s canonical: %s" % (fn, cls))
        pre, sub, high = mont_model(first(a), b)
        assert not high and pre < 2 * R                 # canonical inputs never reach t[8] / t[9]
        assert pre != R                                 # EXEMPT_CLASSES
        count("%s canonical: subtraction %s" % (fn, "taken" if sub else "not taken"))
        if not sub and R - pre <= 1 << 32:
            count("%s canonical: not taken, pre-subtraction value within 2^32 below r" % fn)
        if sub and pre - R < 1 << 32:
            count("%s canonical: taken, pre-subtraction value within 2^32 above r" % fn)
    return out


def out_of_contract_pairs(prng):
    big = list(OUT_OF_CONTRACT) + [prng.randrange(R, 1 << 256) for _ in range(20)]
    out = [("edges", a, b) for a in big for b in big]
    out += [("against canonical", a, b) for a in big for b in (0, 1, R - 1, prng.randrange(R))]
    out += [("against canonical", b, a) for a in big for b in (0, 1, R - 1, prng.randrange(R))]
    out += [("random 256-bit", prng.randrange(1 << 256), prng.randrange(1 << 256)) for _ in range(500)]
    for cls, a, b in out:
        count("mont_mul out of contract: " + cls)
        count("mont_mul out of contract: t[8] / t[9] %s" % ("non-zero" if mont_model(a, b)[2] else "zero"))
    return out


def add_pairs(prng):
    e = canonical_edges()
    out = [("canonical edges", a, b) for a in e for b in e]
    for _ in range(100):
        a = prng.randrange(1, R)
        out += [("sum equal to r", a, R - a), ("sum r + 1", a, R - a + 1) if a > 1 else ("sum equal to r", a, R - a),
                ("sum r - 1", a, R - a - 1)]
    out += [("sum 2r - 2", R - 1, R - 1), ("sum below r", 0, 0), ("sum below r", 0, R - 1), ("sum equal to r", 1, R - 1)]
    for i in range(1, 8):                               # the carry of the addition through every word boundary
        low = (1 << (32 * i)) - 1
        for high in (0, prng.randrange(R >> (32 * i)) << (32 * i)):
            out += [("carry through a word boundary", high + low, 1), ("carry through a word boundary", 1, high + low),
                    ("carry through a word boundary", high + low, low)]
    # the borrow of the trial subtraction through every word boundary: sums r + x with the low i words of x all ones / zero
    for i in range(1, 8):
        for x in ((1 << (32 * i)) - 1, 1 << (32 * i)):
            a = prng.randrange(x + 1, R)
            out.append(("sum above r, borrow chain", a, R + x - a))
    out += [("random", prng.randrange(R), prng.randrange(R)) for _ in range(N_RANDOM)]
    for cls, a, b in out:
        assert 0 <= a < R and 0 <= b < R, cls
        count("add: " + cls)
        count("add: " + ("wraps" if a + b >= R else "does not wrap"))
    return out


def sub_mul_triples(prng):
    e = canonical_edges()
    out = [("canonical edges", a, b, c) for a in e for b in e for c in e]
    for _ in range(300):
        b, c = prng.randrange(1, R), prng.randrange(1, R)
        bc = b * c % R
        out += [("a equal to b c", bc, b, c), ("a = b c + 1: no borrow", (bc + 1) % R, b, c), ("a = b c - 1: add-back", (bc - 1) % R, b, c),
                ("a = 0", 0, b, c)]
    for _ in range(50):
        a, x = prng.randrange(R), prng.randrange(R)
        out += [("b c = 0", a, 0, x), ("b c = 0", a, x, 0)]
    taken = 0
    while taken < 300:                                  # the inner product takes its final subtraction
        b, c = prng.randrange(R), prng.randrange(R)
        if mont_model(b * (1 << 256) % R, c)[1]:
            out.append(("inner product takes the final subtraction", prng.randrange(R), b, c))
            taken += 1
    out += [("random", prng.randrange(R), prng.randrange(R), prng.randrange(R)) for _ in range(N_RANDOM)]
    for cls, a, b, c in out:
        assert max(a, b, c) < R
        count("sub_mul: " + cls)
        bc = b * c % R
        count("sub_mul: " + ("a >= b c, no borrow" if a >= bc else "a < b c, add-back"))
        if a == bc:
            count("sub_mul: difference 0")
        if a == 0:
            count("sub_mul: a zero")
        if bc == 0:
            count("sub_mul: b c zero")
    return out


def half_cases(prng):
    top = (1 << 126) - 1
    out = [("u = 0, b < 0", 1, 1, 0), ("u = 0, b < 0", top, 1, 0), ("u = 0", top, 0, 0),
           ("|b| = 2^126 - 1, u = r - 1", top, 0, R - 1), ("|b| = 2^126 - 1, u = r - 1", top, 1, R - 1)]
    out += [("random", prng.randrange(1, 1 << 126), prng.randrange(2), prng.randrange(R)) for _ in range(50)]
    # u >= r (a malformed item; the product discards the result): through fr_mont_mul out of its contract.  Only b >= 0:
    # for b < 0 the function returns r - w, which borrows when w >= r and then means nothing
    out += [("out of contract: u >= r", m, 0, u) for u in OUT_OF_CONTRACT + (prng.randrange(R, 1 << 256),) for m in (1, top, prng.randrange(1, 1 << 126))]
    for cls, *_ in out:
        count("half_scalar_times_u: " + cls)
    return out


def truncate_cases(prng):
    xs = [("0, 1, q - 1", x) for x in (0, 1, Q - 1)] + [("around 2^250", x) for x in ((1 << 250) - 1, 1 << 250, (1 << 250) + 1)]
    xs += [("2^k, k = 248 .. 254", 1 << k) for k in range(248, 255)] + [("all ones below q", (1 << 254) - 1)]
    xs += [("random", prng.randrange(Q)) for _ in range(500)]
    out = []
    for cls, x in xs:
        assert 0 <= x < Q
        for rep in (0, 1):                              # fe_n: value below 2q, so two representatives of a residue
            out.append((cls, x, rep))
            count("truncate250: %s, representative %d" % (cls, rep))
            count("truncate250: bits 250 .. 254 " + ("set" if x >> 250 else "clear"))
    return out


def chacha_cases(prng):
    v = check_chacha20_against_rfc()
    out = [("RFC 8439 2.3.2", bytes.fromhex(v["key"]), v["counter"], bytes.fromhex(v["nonce"]))]
    nonce = prng.randbytes(12)
    for name, key in (("all-zero key", bytes(32)), ("all-ones key", b"\xff" * 32)):
        for ctr in (0, 1, 1 << 31, M32):
            out += [(name, key, ctr, bytes(12)), (name, key, ctr, b"\xff" * 12), (name, key, ctr, nonce)]
    out += [("counter edges", prng.randbytes(32), ctr, prng.randbytes(12)) for ctr in (0, 1, 1 << 31, M32)]
    out += [("random", prng.randbytes(32), prng.randrange(1 << 32), prng.randbytes(12)) for _ in range(200)]
    for cls, *_ in out:
        count("chacha20: " + cls)
    return out


def weight_cases(prng):
    seeds = [("pinned seed", PINNED_SEED)] + [("random seed", prng.randbytes(32)) for _ in range(3)]
    out = []
    for bits in range(128, 161):
        top = [False, False]
        for cls, seed in seeds:
            for item in WEIGHT_ITEMS:
                out.append((cls, seed, item, bits))
                count("weights: " + cls)
                count("weights: item %s 2^32" % ("from" if item >> 32 else "below"))
                z, zp = weights(seed, item, bits)
                top = [top[0] or bool(z >> (bits - 1)), top[1] or bool(zp >> (bits - 1))]
        assert all(top), bits                           # the expectation itself has the top kept bit set in z and in z'
        count("weights: bits %s multiple of 32" % ("a" if bits % 32 == 0 else "no"))
    return out


# ---- records ---------------------------------------------------------------------------------------------------------------
def w8(x, n=8):
    return np.frombuffer(int(x).to_bytes(4 * n, "little"), np.uint32)


def _val(words):
    return int.from_bytes(np.ascontiguousarray(words, dtype=np.uint32).tobytes(), "little")


def _rec(kind, cases, rows):
    words_in, _ = SHAPE[kind]
    arr = np.zeros((len(cases), words_in), np.uint32)
    for i, r in enumerate(rows):
        arr[i, :len(r)] = r
    return {"kind": kind, "cases": cases, "in": arr}


@functools.lru_cache(maxsize=1)
def _build():
    CLASS_COUNTS.clear()
    prng = random.Random(610)
    recs = {}
    for name, kind, fn in (("mont_mul", "K_MONT_MUL", "mont_mul"), ("mul", "K_MUL", "mul")):
        c = product_pairs(prng, fn)
        recs[name] = _rec(kind, c, [np.concatenate([w8(a), w8(b)]) for _, a, b in c])
    c = out_of_contract_pairs(prng)
    recs["mont_mul out of contract"] = _rec("K_MONT_MUL", c, [np.concatenate([w8(a), w8(b)]) for _, a, b in c])
    c = sub_mul_triples(prng)
    recs["sub_mul"] = _rec("K_SUB_MUL", c, [np.concatenate([w8(a), w8(b), w8(x)]) for _, a, b, x in c])
    c = add_pairs(prng)
    recs["add"] = _rec("K_ADD", c, [np.concatenate([w8(a), w8(b)]) for _, a, b in c])
    c = half_cases(prng)
    recs["half_scalar_times_u"] = _rec("K_HALF_TIMES_U", c, [np.concatenate([w8(m, 4), w8(neg, 4), w8(u)]) for _, m, neg, u in c])
    c = truncate_cases(prng)
    recs["truncate250"] = _rec("K_TRUNCATE250", c, [np.concatenate([w8(x), w8(rep, 1)]) for _, x, rep in c])
    c = chacha_cases(prng)
    recs["chacha20"] = _rec("K_CHACHA20", c, [np.concatenate([np.frombuffer(k, np.uint32), w8(ctr, 1), np.frombuffer(n, np.uint32)]) for _, k, ctr, n in c])
    c = weight_cases(prng)
    recs["weights"] = _rec("K_WEIGHTS", c, [np.concatenate([np.frombuffer(s, np.uint32), w8(item, 2), w8(bits, 1)]) for _, s, item, bits in c])
    return recs, dict(CLASS_COUNTS)


def build_records():
    """{name: record}, in the order the executors run them; CLASS_COUNTS is filled as a side effect (built once a session)"""
    recs, counts = _build()
    CLASS_COUNTS.clear()
    CLASS_COUNTS.update(counts)
    return {k: dict(v) for k, v in recs.items()}


def input_words(recs):
    parts = []
    for r in recs.values():
        parts += [np.array([KIND[r["kind"]] << 24, len(r["cases"])], np.uint32), r["in"].reshape(-1)]
    return np.concatenate(parts)


def output_words(recs):
    return sum(len(r["cases"]) * SHAPE[r["kind"]][1] for r in recs.values())


def attach_outputs(recs, out):
    at = 0
    for r in recs.values():
        n, w = len(r["cases"]), SHAPE[r["kind"]][1]
        r["out"] = out[at:at + n * w].reshape(n, w)
        at += n * w
    assert at == len(out)
    return recs


# ---- checks ----------------------------------------------------------------------------------------------------------------
def _check(rec, want):
    """every output row of `rec` against want(case) -> the expected integer of the first 8 words"""
    bad = []
    for i, case in enumerate(rec["cases"]):
        got = _val(rec["out"][i, :8])
        if got != want(*case[1:]):
            bad.append((case[0],) + tuple(hex(x) if isinstance(x, int) else x for x in case[1:]) + (hex(got),))
    assert not bad, (len(bad), bad[:5])


def check_mont_mul(recs):
    _check(recs["mont_mul"], lambda a, b: a * b * R_INV256 % R)
    rec = recs["mont_mul out of contract"]
    ge_r = 0
    for i, (cls, a, b) in enumerate(rec["cases"]):
        got = _val(rec["out"][i])
        assert got % R == a * b * R_INV256 % R, (cls, hex(a), hex(b), hex(got))      # congruent, in 256 bits
        ge_r += got >= R
    OUT_OF_CONTRACT_GE_R["mont_mul"] = (ge_r, len(rec["cases"]))


def check_mul(recs):
    _check(recs["mul"], lambda a, b: a * b % R)


def check_sub_mul(recs):
    _check(recs["sub_mul"], lambda a, b, c: (a - b * c) % R)


def check_add(recs):
    _check(recs["add"], lambda a, b: (a + b) % R)


def check_half(recs):
    rec = recs["half_scalar_times_u"]
    for i, (cls, m, neg, u) in enumerate(rec["cases"]):
        got = _val(rec["out"][i])
        want = (-m if neg else m) * u % R
        if u >= R:
            assert got % R == want, (cls, hex(m), hex(u), hex(got))
        else:
            assert got == want, (cls, hex(m), neg, hex(u), hex(got))


def check_truncate250(recs):
    rec = recs["truncate250"]
    _check(rec, lambda x, rep: x % (1 << 250))
    for i, (cls, x, rep) in enumerate(rec["cases"]):
        assert int(rec["out"][i, 8]) == rep, (cls, hex(x), rep)      # the second representative has other limbs


def check_chacha20(recs):
    rec = recs["chacha20"]
    for i, (cls, key, ctr, nonce) in enumerate(rec["cases"]):
        assert rec["out"][i].tobytes() == chacha20_block(key, ctr, nonce), (cls, key.hex(), ctr, nonce.hex())


def check_weights(recs):
    rec = recs["weights"]
    for i, (cls, seed, item, bits) in enumerate(rec["cases"]):
        z, zp = weights(seed, item, bits)
        assert (_val(rec["out"][i, :8]), _val(rec["out"][i, 8:])) == (z, zp), (cls, seed.hex(), item, bits)


def classes_populated():
    assert CLASS_COUNTS and all(v > 0 for v in CLASS_COUNTS.values()), CLASS_COUNTS
    need = ["%s canonical: %s" % (fn, c) for fn in ("mont_mul", "mul")
            for c in ("canonical edges", "random", "subtraction taken", "subtraction not taken",
                      "not taken, pre-subtraction value within 2^32 below r", "taken, pre-subtraction value within 2^32 above r")]
    need += ["%s canonical: weight-shaped %d bits x %s" % (fn, b, x) for fn in ("mont_mul", "mul") for b in WEIGHT_BITS for x in "cu"]
    need += ["mont_mul out of contract: " + c for c in ("edges", "against canonical", "random 256-bit", "t[8] / t[9] non-zero")]
    need += ["add: " + c for c in ("sum below r", "sum equal to r", "sum r + 1", "sum 2r - 2", "carry through a word boundary",
                                   "sum above r, borrow chain", "wraps", "does not wrap", "random")]
    need += ["sub_mul: " + c for c in ("a >= b c, no borrow", "a < b c, add-back", "difference 0", "a zero", "b c zero",
                                       "inner product takes the final subtraction", "canonical edges", "random")]
    need += ["half_scalar_times_u: " + c for c in ("u = 0, b < 0", "|b| = 2^126 - 1, u = r - 1", "out of contract: u >= r")]
    need += ["truncate250: %s, representative %d" % (c, rep) for rep in (0, 1)
             for c in ("0, 1, q - 1", "around 2^250", "2^k, k = 248 .. 254", "all ones below q", "random")]
    need += ["chacha20: " + c for c in ("RFC 8439 2.3.2", "all-zero key", "all-ones key", "counter edges", "random")]
    need += ["weights: " + c for c in ("pinned seed", "random seed", "item from 2^32", "item below 2^32", "bits a multiple of 32")]
    missing = [c for c in need if CLASS_COUNTS.get(c, 0) == 0]
    assert not missing, missing
    for fn in ("mont_mul", "mul"):
        assert CLASS_COUNTS["%s canonical: final subtraction taken (random search)" % fn] >= 300
        assert CLASS_COUNTS["%s canonical: not taken, pre-subtraction value within 2^32 below r" % fn] >= 300
    assert CLASS_COUNTS["mont_mul canonical: random"] == CLASS_COUNTS["sub_mul: random"] == CLASS_COUNTS["add: random"] == N_RANDOM
    assert all(c not in CLASS_COUNTS for c in EXEMPT_CLASSES)

"""The generated blocks of csrc/mont_asm.inc (tools/gen_mont_asm.py) -- the Montgomery product and square of fq29.h and the Hades
linear layer of hades29.h -- interpreted instruction by instruction on the CPU.  Limb vectors go in as they are, with no round
trip through their value, at the edges of every bound class that a static_assert admits for a caller of the block: random
limbs, every limb at its maximum, the top limb at its maximum (the value clamped below A q).  The square also takes what
hades29.h gives it without a carry pass: normalised limbs plus each Hades round constant, read from csrc/jjs_constants.inc.
The checks are what the callers rely on: the value a * b / 2^261 mod q (the linear layer: sum_j S[i+j] t_j / 2^29 mod q),
limbs 0..7 below 2^29, a value in (0, 2q), and in [1, q] for a product with the constant 1 (fq_canon_limbs).  The register
tests check that no block reads a register before writing it, that it writes only its outputs and its clobber list, and that
every output operand in fq29.h / hades29.h is early-clobber.  A mistake in the generator shows up here, without a GPU.  (Round 4
also generated a latency variant of both products -- the column sums gathered in a ring of eight accumulators, three dependent
instructions a column instead of one chain of 189 -- and this interpreter showed it limb-for-limb equal; on the device it was 4 %
SLOWER for the hash lanes it was meant for, profiles/r04_latency_blocks_ab.jsonl, and was removed.)"""
import os
import random
import re

import numpy as np
import pytest

from helpers import const_table, edge_limb_vectors, limbs_val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jubjub_schnorr_amd", "csrc")
Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
RINV = pow(1 << 261, -1, Q)
INV29 = pow(1 << 29, -1, Q)
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
M29 = (1 << 29) - 1


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def macro(text, name):
    """The body of `#define name ...`, continuation lines joined."""
    start = re.search(r"^#define %s\b" % name, text, re.M)
    assert start, name
    body = []
    for line in text[start.end():].splitlines():
        body.append(line[:-1] if line.endswith("\\") else line)
        if not line.endswith("\\"):
            break
    return "\n".join(body)


def blocks():
    text = source("mont_asm.inc")
    return {name: re.findall(r'"(.*?)\\n\\t"', macro(text, name))
            for name in ("JJS_MONT_MUL_ASM", "JJS_MONT_SQR_ASM", "JJS_HADES_MATRIX_ASM")}


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def operand(text):
    m = re.match(r"([sv])\[(\d+):(\d+)\]$", text)
    if m:
        lo, hi = int(m.group(2)), int(m.group(3))
        assert hi == lo + 1, text
        return ("pair", m.group(1) + str(lo), m.group(1) + str(hi))
    if re.match(r"^-?(0x[0-9a-fA-F]+|\d+)$", text):
        return ("imm", int(text, 0))
    return ("reg", text)


def parse(lines):
    prog = []
    for line in lines:
        op, rest = line.split(None, 1)
        prog.append((op, [operand(x.strip()) for x in re.split(r",\s*(?![^\[]*\])", rest)]))
    return prog


class Machine:
    """Registers hold 32-bit values; a register read before it is written raises KeyError."""

    def __init__(self, regs):
        self.r = dict(regs)
        self.written = set()

    def get(self, x):
        if x[0] == "imm":
            return x[1]
        if x[0] == "pair":
            return self.r[x[1]] | (self.r[x[2]] << 32)
        return self.r[x[1]]

    def put(self, x, val):
        if x[0] == "pair":
            self.r[x[1]], self.r[x[2]] = val & M32, (val >> 32) & M32
            self.written.update((x[1], x[2]))
        else:
            assert x[0] == "reg", x
            self.r[x[1]] = val & M32
            self.written.add(x[1])

    def run(self, prog):
        g = self.get
        for op, a in prog:
            if op == "s_mov_b32":
                self.put(a[0], g(a[1]))
            elif op == "s_mov_b64":
                self.put(a[0], g(a[1]) & M64)
            elif op == "v_lshlrev_b32":
                self.put(a[0], g(a[2]) << g(a[1]))
            elif op == "v_mad_u64_u32":            # dst, vcc, x, y, addend
                self.put(a[0], ((g(a[2]) & M32) * (g(a[3]) & M32) + g(a[4])) & M64)
                self.put(a[1], 0)
            elif op == "v_mad_i64_i32":
                self.put(a[0], (s32(g(a[2])) * s32(g(a[3])) + g(a[4])) & M64)
                self.put(a[1], 0)
            elif op == "v_lshl_add_u64":           # dst, x, shift, addend
                self.put(a[0], ((g(a[1]) << g(a[2])) + g(a[3])) & M64)
            elif op == "v_and_b32":
                self.put(a[0], g(a[1]) & g(a[2]))
            elif op == "v_add_u32":
                self.put(a[0], g(a[1]) + g(a[2]))
            elif op == "v_sub_u32":
                self.put(a[0], g(a[1]) - g(a[2]))
            elif op == "v_ashrrev_i64":
                self.put(a[0], s64(g(a[2])) >> g(a[1]))
            elif op == "v_lshrrev_b64":
                self.put(a[0], (g(a[2]) & M64) >> g(a[1]))
            elif op == "v_alignbit_b32":           # dst, hi, lo, shift: (hi:lo) >> shift, low 32 bits
                self.put(a[0], (((g(a[1]) & M32) << 32) | (g(a[2]) & M32)) >> g(a[3]))
            else:
                raise ValueError(op)
        return self


PROG = {k: parse(v) for k, v in blocks().items()}
HANKEL = const_table("JJS_HS_HANKEL")
HADES_CONSTS = const_table("JJS_HS_RC_FULL") + const_table("JJS_HS_KAPPA")


def limbs(x):
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> (29 * 8)]


def mont_mul(a, b):
    regs = {"%%[a%d]" % i: int(a[i]) for i in range(9)}
    regs.update({"%%[b%d]" % i: int(b[i]) for i in range(9)})
    m = Machine(regs).run(PROG["JJS_MONT_MUL_ASM"])
    return [m.r["%%[a%d]" % i] for i in range(9)]


def mont_sqr(a):
    m = Machine({"%%[a%d]" % i: int(a[i]) for i in range(9)}).run(PROG["JJS_MONT_SQR_ASM"])
    return [m.r["%%[a%d]" % i] for i in range(9)]


def hades_matrix(t):
    regs = {"%%[t%d_%d]" % (j, c): int(t[j][c]) for j in range(5) for c in range(9)}
    regs.update({"%%[h%d]" % k: HANKEL[k] for k in range(9)})
    m = Machine(regs).run(PROG["JJS_HADES_MATRIX_ASM"])
    return [[m.r["%%[o%d_%d]" % (i, c)] for c in range(9)] for i in range(5)]


def check_product(got, want, what):
    v = limbs_val(got)
    assert all(x < 1 << 29 for x in got[:8]), what
    assert 0 < v < 2 * Q, what
    assert v % Q == want % Q, what


def test_blocks_compute_the_montgomery_product():
    B = blocks()
    assert len(B["JJS_MONT_MUL_ASM"]) == 189 + 8 and len(B["JJS_MONT_SQR_ASM"]) == 161 + 8      # + the 8 s_mov of the prologue
    assert len(B["JJS_HADES_MATRIX_ASM"]) == 374
    rng = random.Random(29)
    cases = [(rng.randrange(2 * Q), rng.randrange(2 * Q)) for _ in range(300)]
    cases += [(0, 0), (1, 1), (Q - 1, Q - 1), (2 * Q - 1, 2 * Q - 1), (Q, 5), ((1 << 255) - 1, (1 << 255) - 1)]
    for x, y in cases:
        check_product(mont_mul(limbs(x), limbs(y)), x * y * RINV, (x, y))
        check_product(mont_sqr(limbs(x)), x * x * RINV, x)
    # limbs up to 3 * 2^29 - 1 on one side, fed in as they are (fq_mul: La * Lb <= 3)
    for _ in range(50):
        wide = [rng.randrange(3 << 29) for _ in range(8)] + [rng.randrange(1 << 24)]
        y = rng.randrange(2 * Q)
        check_product(mont_mul(wide, limbs(y)), limbs_val(wide) * y * RINV, wide)
        check_product(mont_mul(limbs(y), wide), limbs_val(wide) * y * RINV, wide)


# value bounds (Aa, Ab) tried for every limb class; fq_mul / fq_mul_hot admit La * Lb <= 3, fq_mul_chain La * Lb <= 4
VALUE_PAIRS = ((2, 2), (1, 70), (70, 1), (2, 35), (35, 2), (7, 10), (10, 7), (8, 8))
PRODUCT_CLASSES = [((1, 1), "fq_mul / fq_mul_hot"), ((1, 3), "fq_mul / fq_mul_hot"), ((3, 1), "fq_mul / fq_mul_hot"),
                   ((2, 2), "fq_mul_chain"), ((1, 4), "fq_mul_chain"), ((4, 1), "fq_mul_chain")]


@pytest.mark.parametrize("lab,caller", PRODUCT_CLASSES, ids=["%dx%d" % c[0] for c in PRODUCT_CLASSES])
def test_product_block_at_the_edges_of_every_bound_class(lab, caller):
    la, lb = lab
    rng = np.random.default_rng(100 * la + lb)
    for aa, ab in VALUE_PAIRS:
        assert la * lb <= 4 and aa * ab <= 70
        a, b = edge_limb_vectors(rng, 24, la, aa), edge_limb_vectors(rng, 24, lb, ab)
        for x, y in zip(a, b):
            check_product(mont_mul(x, y), limbs_val(x) * limbs_val(y) * RINV, (caller, la, aa, lb, ab, x.tolist(), y.tolist()))


def test_square_block_of_normalised_operands():
    """fq_sqr / fq_sqr_hot / fq_sqr_chain: La = 1, Aa * Aa <= 70"""
    rng = np.random.default_rng(11)
    for aa in (1, 2, 4, 8):
        for x in edge_limb_vectors(rng, 48, 1, aa):
            check_product(mont_sqr(x), limbs_val(x) ** 2 * RINV, (aa, x.tolist()))


def test_blocks_on_normalised_limbs_plus_each_hades_constant():
    """fq_sqr_plus_const / fq_sqr_chain square (fe_n + constant) with limbs up to 2^30 - 1 and no carry pass, and fq_mul_chain
    multiplies such a value by itself and by a normalised value: exact only because of the constants' own limbs.  Every
    constant of JJS_HS_RC_FULL and JJS_HS_KAPPA, on fe_n operands at their edges."""
    assert len(HADES_CONSTS) == 8 * 5 + 60
    rng = np.random.default_rng(12)
    ns = edge_limb_vectors(rng, 8, 1, 2)
    ms = edge_limb_vectors(rng, 8, 1, 2)
    for k, c in enumerate(HADES_CONSTS):
        assert all(x < 1 << 29 for x in c) and limbs_val(c) < Q
        for n, m in zip(ns, ms):
            x = [int(n[i]) + c[i] for i in range(9)]                   # fe<2, 3>
            v = limbs_val(x)
            check_product(mont_sqr(x), v * v * RINV, ("sqr", k, n.tolist()))
            check_product(mont_mul(x, x), v * v * RINV, ("mul x x", k, n.tolist()))
            check_product(mont_mul(m, x), limbs_val(m) * v * RINV, ("mul n x", k, n.tolist()))


def test_product_with_one_lands_in_1_to_q():
    """fq_canon_limbs takes fq_mul(fq_norm(a), 1) in [1, q], with q standing for zero, for every value bound up to 70 q"""
    rng = np.random.default_rng(13)
    one = [1] + [0] * 8
    for aa in (1, 2, 3, 4, 5, 9, 35, 70):
        cases = [list(map(int, x)) for x in edge_limb_vectors(rng, 32, 1, aa)]
        cases += [limbs(k * Q + d) for k in range(aa) for d in (-1, 0, 1) if 0 <= k * Q + d < aa * Q]
        for x in cases:
            got = mont_mul(x, one)
            v = limbs_val(got)
            assert all(l < 1 << 29 for l in got[:8]) and 1 <= v <= Q, (aa, x)
            assert v % Q == limbs_val(x) * RINV % Q, (aa, x)
            assert limbs_val(mont_mul(one, x)) == v, (aa, x)
    assert limbs_val(mont_mul([0] * 9, one)) == Q


def hankel_residue_states(rng, n):
    """fe_n states whose first column of row i sums to 0, 1, 2, -2 or -1 mod 2^29 (rows 0..3: through t_{3-i}, whose
    coefficient 45045 is odd; row 4's coefficients are all even), where the rounding of the first quotient digit shows"""
    inv = pow(HANKEL[3], -1, 1 << 29)
    out = []
    base = edge_limb_vectors(rng, 5 * n, 1, 2).reshape(n, 5, 9)
    for s in range(n):
        t = [list(map(int, base[s, j])) for j in range(5)]
        i, r = s % 4, (0, 1, 2, M29 - 1, M29)[s % 5]
        j = 3 - i
        rest = sum(HANKEL[i + k] * t[k][0] for k in range(5) if k != j)
        t[j][0] = (r - rest) * inv % (1 << 29)
        if limbs_val(t[j]) < 2 * Q:
            out.append(t)
    return out


def test_hades_matrix_block_rows():
    """JJS_HADES_MATRIX_ASM: row i is sum_j S[i+j] t_j / 2^29 mod q (S[i][j] = JJS_HS_HANKEL[i + j]) for t at the fe_n edges,
    with normalised limbs and a value below 2q"""
    assert HANKEL == [360360 // (k + 5) for k in range(9)]
    rng = np.random.default_rng(14)
    ts = [[list(map(int, t[j])) for j in range(5)] for t in np.stack([edge_limb_vectors(rng, 48, 1, 2) for _ in range(5)], axis=1)]
    ts += [[[0] * 9] * 5, [limbs(2 * Q - 1)] * 5, [limbs(Q)] * 5] + hankel_residue_states(rng, 40)
    for t in ts:
        tv = [limbs_val(t[j]) for j in range(5)]
        rows = hades_matrix(t)
        for i in range(5):
            v = limbs_val(rows[i])
            assert all(x < 1 << 29 for x in rows[i][:8]), (i, t)
            assert v < 2 * Q, (i, t)
            assert v % Q == sum(HANKEL[i + j] * tv[j] for j in range(5)) * INV29 % Q, (i, t)


# ---- registers ------------------------------------------------------------------------------------------------------------
def asm_statements():
    """(header, block, outputs {name: constraint}, inputs [name], clobbers [register]) of every asm statement in fq29.h and
    hades29.h, operand macros expanded from mont_asm.inc"""
    inc = source("mont_asm.inc")
    out = []
    for header in ("fq29.h", "hades29.h"):
        for m in re.finditer(r"\basm\s*\(\s*(JJS_\w+)(.*?)\);", source(header), re.S):
            sections = m.group(2).split(":")
            assert len(sections) == 4 and not sections[0].strip(), (header, m.group(1))
            sections = [macro(inc, s.strip()) if re.match(r"^JJS_\w+$", s.strip()) else s for s in sections[1:]]
            outs = dict(re.findall(r'\[(\w+)\]\s*"([^"]+)"', sections[0]))
            ins = re.findall(r'\[(\w+)\]\s*"[^"]+"', sections[1])
            clobbers = re.findall(r'"([^"]+)"', sections[2])
            out.append((header, m.group(1), outs, ins, clobbers))
    return out


def test_no_register_is_read_before_it_is_written():
    """the interpreter raises KeyError on such a read; write-only (=) outputs start unset"""
    for header, name, outs, ins, _ in asm_statements():
        regs = {"%%[%s]" % k: 12345 + i for i, k in enumerate(ins)}
        regs.update({"%%[%s]" % k: 777 + i for i, k in enumerate(outs) if outs[k].startswith("+")})
        Machine(regs).run(PROG[name])


def test_blocks_write_only_outputs_and_clobbers():
    stmts = asm_statements()
    assert sorted(s[1] for s in stmts) == sorted(["JJS_MONT_MUL_ASM"] * 2 + ["JJS_MONT_SQR_ASM"] * 2 + ["JJS_HADES_MATRIX_ASM"])
    for header, name, outs, ins, clobbers in stmts:
        regs = {"%%[%s]" % k: 12345 + i for i, k in enumerate(ins)}
        regs.update({"%%[%s]" % k: 777 + i for i, k in enumerate(outs)})
        written = Machine(regs).run(PROG[name]).written
        for r in written:
            m = re.match(r"%\[(\w+)\]$", r)
            if m:
                assert m.group(1) in outs, (header, name, r)          # never an input operand
            else:
                assert r in clobbers, (header, name, r)
        # every output is written (an output left as it came in would hand back an input)
        assert all("%%[%s]" % k in written for k in outs), (header, name)


def test_asm_outputs_are_early_clobber():
    """the blocks write outputs while inputs are still to be read: no output may share a register with an input"""
    for header, name, outs, _, _ in asm_statements():
        assert outs, (header, name)
        for k, c in outs.items():
            assert c in ("+&v", "=&v"), (header, name, k, c)

"""The digit function of the key-table path and the first addition of its sums, on the CPU build
(tests/hostbuild/key_digits_harness.cpp).

kt_digit and comb_digit are one function over two sources: the registers of a lane (every caller but one) and the
[word][lane] array key_verify_kernel keeps in LDS.  Both must give, for every position and both window widths, what the
extraction gave while it stood in line in kt_add_digit / add_comb_range (the harness keeps that text), and for scalars in
range the textbook digits of tests/scalar_mul_cases.py.  kt_first_entry, which starts a sum from the top position's entry,
must be the point that identity + entry is, for every digit of a position: 0 and both signs, as affine points against the
Python oracle, with a valid T (the next addition multiplies by it)."""
import ctypes
import os
import random

import numpy as np
import pytest

import jjs_oracle as o
import scalar_mul_cases as smc
from hostlib import build_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostbuild", "key_digits_harness.cpp")
LIB = os.path.join(HERE, "hostbuild", "libjjs_key_digits.so")
R = o.R_ORDER
# the last three are malformed: all-ones words, and two whose top digit is beyond the narrow windows' table
NAMED = [0, 1, R - 1, (1 << 250) - 1, (1 << 252) - 1, (1 << 256) - 1, (15 << 252) + 12345, 1 << 255]


@pytest.fixture(scope="module")
def lib():
    return build_hostlib(SRC, LIB)


@pytest.fixture(scope="module")
def scalars():
    prng = random.Random(0xD161)
    return NAMED + [prng.randrange(1 << 252) for _ in range(1000)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("w", [5, 6])
def test_digits_from_registers_from_lanes_and_in_line(lib, scalars, w):
    n, positions, windows = len(scalars), lib.jjs_kd_positions(w), lib.jjs_kd_comb_windows()
    assert positions == smc.positions(w) and windows == 16
    words = np.array([smc.w8(s) for s in scalars], np.uint32)
    regs, lanes, in_line = (np.full((n, positions), 99, np.int32) for _ in range(3))
    comb = [np.full((n, windows), 0xFFFFFFFF, np.uint32) for _ in range(3)]
    assert lib.jjs_kd_digits(_p(words), ctypes.c_size_t(n), w, _p(regs), _p(lanes), _p(in_line), *[_p(c) for c in comb]) == 0
    assert (regs == in_line).all() and (lanes == in_line).all()
    assert (comb[0] == comb[2]).all() and (comb[1] == comb[2]).all()
    last = 1 << (w - 1)
    assert np.abs(in_line).max() <= last                       # inside the table, the malformed scalar too
    for i, s in enumerate(scalars):
        assert comb[0][i].tolist() == smc.digits(s, 16), hex(s)
        if s < 1 << 252:
            assert regs[i].tolist() == smc.digits(s, w), (w, hex(s))
    # malformed scalars: the sum with the recoding constant is taken modulo 2^256, and a top digit beyond the table is clamped
    clamped = 0
    for i, s in enumerate(scalars):
        t = (s + smc.recode_constant(w)) % (1 << 256)
        top = t >> (w * (positions - 1))
        clamped += top > last
        want = [((t >> (w * p)) & ((1 << w) - 1)) - last for p in range(positions - 1)] + [min(top, last)]
        assert regs[i].tolist() == want, (w, hex(s))
    assert clamped or w == 6                   # four bits are left above bit 252: the wide windows' top digit is always in range
    # every digit value occurs at a position below the top, and a non-zero top digit occurs: the comparison is not vacuous
    assert set(np.unique(regs[:, :-1]).tolist()) == set(range(-last, last))
    assert regs[:, -1].max() > 0


@pytest.mark.parametrize("w", [5, 6])
def test_first_entry_is_identity_plus_entry(lib, w):
    prng = random.Random(0xF125 + w)
    last = 1 << (w - 1)
    for base in (o.G, o.mul(o.G_NUMS, prng.randrange(1, R))):
        first, added = (np.full((2 * last + 1, 36), 0xFFFFFFFF, np.uint32) for _ in range(2))
        assert lib.jjs_kd_first_entry(_p(np.array(smc.pt16(base), np.uint32)), w, _p(first), _p(added)) == 0
        for j, d in enumerate(range(-last, last + 1)):
            want = o.mul(base, d) if d >= 0 else o.neg(o.mul(base, -d))
            smc.check_point(added[j], want, ("identity + entry", w, d))
            smc.check_point(first[j], want, ("first entry", w, d))           # bounds of fe_n, the affine point, T Z == X Y
        assert o.mul(base, 0) == o.IDENTITY

"""Poseidon digests of ragged inputs on the CPU build: the functions of csrc/digest.h -- the code of the device's one-lane-per-item
route -- over the case lists of digest_cases.py, against oracle poseidon_any and poseidon_digest, bit for bit: every digest, every
status, the zeroed rows.  The eight-lane route is device-only.  No GPU."""
import numpy as np
import pytest

import digest_cases as dc
import digest_hostlib as hl
import jjs_oracle as o


def check(case, flags=0, ordered=True, want_status=True):
    rc, out, status = hl.digest(case, flags, ordered, want_status)
    assert rc == 0
    want = dc.truncated(case["want"]) if flags & 1 else case["want"]
    rows = np.where((out != want).any(1))[0]
    assert len(rows) == 0, (rows[:8], case["status"][rows[:8]])
    if want_status:
        assert (status == case["status"]).all(), np.where(status != case["status"])[0][:8]
    return out


# (the sizes are those of the device's waves and mean nothing to one CPU thread: the lengths beyond 1 000 elements, 258 permutations
# an item, run at two of them)
@pytest.mark.parametrize("k,n", [(k, n) for k in dc.LENGTHS for n in (dc.SIZES if k < 1000 else (1, 65))])
def test_uniform_lengths(k, n):
    case = dc.uniform(k, n)
    full = check(case)
    cut = check(case, flags=1)
    assert (cut[:, 31] <= 3).all() and (cut[:, :31] == full[:, :31]).all()
    for i in {0, n - 1}:
        if k <= 17 or n == 1:
            assert (full[i] == dc.python_digest(case["values"], case["offs"], i)).all()


def test_truncation_is_the_low_250_bits():
    case = dc.uniform(5, 65)
    for row_full, row_cut in zip(check(case), check(case, flags=1)):
        assert dc.to_int(row_cut) == dc.to_int(row_full) & dc.MASK250


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("ordered", [False, True])
def test_ragged(reverse, ordered):
    case = dc.ragged(reverse)
    out = check(case, ordered=ordered)
    check(case, flags=1, ordered=ordered)
    at = case["n"] - 1 - 7 if reverse else 7
    assert case["offs"][at + 1] - case["offs"][at] == 1031
    for i in (0, 3, at):
        assert (out[i] == dc.python_digest(case["values"], case["offs"], i)).all()


def test_equal_lengths_through_offsets_equal_the_uniform_call():
    case = dc.uniform(5, 65)
    a = check(case)
    b = check(dc.as_offsets(case))
    assert a.tobytes() == b.tobytes()


def test_range_test():
    case = dc.range_test()
    assert (case["status"] == 3).sum() == 3 * (1 + 3 + 4) and (case["want"][case["status"] == 3] == 0).all()
    check(case)
    check(case, flags=1)
    check(case, want_status=False)           # status == NULL still zeroes the row


def test_wide():
    case = dc.wide()
    check(case)
    check(case, flags=1)
    assert (case["status"] == 0).all()


def test_wide_elements_one_by_one():
    """lo + 2^256 hi through dg_element against Python integers; the constant is the Montgomery form of 2^256"""
    assert dc.to_int(hl.two256()) == (1 << 256) % o.Q
    rng = np.random.default_rng(5)
    values = list(dc.WIDE_EDGES) + [(1 << 256) - 1, ((1 << 256) - 1) << 256, o.Q - 1, (o.Q - 1) << 256] + \
        [int.from_bytes(rng.bytes(64), "little") for _ in range(64)]
    for x in values:
        bad, out = hl.element(1, dc.le(x, 64))
        assert bad == 0 and dc.to_int(out) == x % o.Q, hex(x)


def test_canonical_elements_one_by_one():
    for x in dc.RANGE_BAD + dc.RANGE_GOOD + (1, o.Q - 2, (1 << 255), (1 << 255) - 1):
        bad, out = hl.element(0, dc.le(x))
        assert bad == (1 if x >= o.Q else 0), hex(x)
        assert dc.to_int(out) == x % o.Q            # the arithmetic is defined on any 256-bit value


@pytest.mark.parametrize("length", [1, 16, 17, 1027, 1028, 1029, 1031, 65536, (1 << 31) - 1])
def test_tags(length):
    """from the table up to 1027, computed beyond: one function of the length"""
    assert dc.to_int(hl.tag(length)) == o.sponge_tag(length)


def test_block_counts_do_not_overflow():
    lib = hl.load()
    for length in (1, 3, 4, 5, (1 << 31) - 4, (1 << 31) - 3, (1 << 31) - 1):
        assert lib.jjs_dg_host_blocks(length) == (length + 3) // 4


def test_order_is_by_block_count_descending_and_stable():
    rng = np.random.default_rng(9)
    shapes = [dc.ragged_lengths(), dc.ragged_lengths()[::-1], [5] * 70, [1], [4, 5], [5, 4], [1, 2, 3, 4] * 9,
              list(rng.integers(1, 3000, 500)), [1, 70000, 3, 300000, 70000, 1 << 20, 5, (1 << 30) + 5, 2]]
    for lens in shapes:
        offsets = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.uint32)
        got = hl.order(offsets)
        assert got.tolist() == dc.block_order(offsets).tolist(), lens[:10]


def test_bad_format_and_flags():
    case = dc.uniform(1, 1)
    for fmt, flags in ((2, 0), (-1, 0), (0, 2), (1, 3)):
        c = dict(case)
        c["fmt"] = fmt
        assert hl.digest(c, flags)[0] == -1

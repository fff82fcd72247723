"""Inputs and checks of the tests of the two verdict algorithms' sums, shared by the CPU build
(test_msm_host.py) and the device (msm_child.py under test_msm_gpu.py): terms for the bucket MSM of csrc/msm.h with scalars
built from digit vectors for every window width from 8 to 16 in both shapes, and index patterns and scalar columns for the run
sums and key points of csrc/keyset_verdict.h.  Every point is k * G with a known k, so an expected sum is ONE o.mul of a sum
of Python integers mod r; the signed digits come from the textbook recoding below, written from the definition in the header of
msm.h.  Nothing here is compared with the host build or with the device.  Every class of case is counted per (width, shape);
CLASS_COUNTS is asserted non-zero class by class, so a change here cannot silently empty one."""
import random

import numpy as np

import jjs_oracle as o
from helpers import fe_arr, pt_arr
from scalar_mul_cases import check_point, from_digits

R = o.R_ORDER
WIDTHS = tuple(range(8, 17))
SHAPES = [(c, short) for c in WIDTHS for short in (False, True)]
MSM_NEG = 1 << 31
KSV_PIECE = 512
CLASS_COUNTS = {}
MSM_CLASSES = ("small", "digits_most_negative", "digits_most_positive", "all_bits_set", "one_digit_low_extreme", "one_digit_high_extreme",
               "one_digit_unit", "largest_top_digit", "random", "same_point_300_one_bucket", "p_and_minus_p_equal_digits",
               "p_digit_d_minus_p_digit_minus_d", "shared_scalar_5000", "n=1", "n=63", "n=64", "n=65", "n=257", "n=4097",
               "kinds 2/0b01", "kinds 4/0b0101", "kinds 3/0b001", "kinds 1/0b1", "kinds 2/0b11")
FULL_ONLY_CLASSES = ("top_every_slot", "r_minus_1")


def count(cls, n=1):
    CLASS_COUNTS[cls] = CLASS_COUNTS.get(cls, 0) + n


# ---- the shapes and the recoding, from the header of msm.h --------------------------------------------------------------------
def shape(c, short):
    """(W, B, s, bound): windows, buckets per window, the top window's split, the scalars' bound.  Full: scalars below 2^252 in
    W = ceil(253 / c) windows, the top digit at most 2^(c-1-s) with s = cW - 253, each top digit split in 2^s slots by the term
    index; short: weights of cW - 1 bits in W = ceil(129 / c) windows, no split."""
    if short:
        W = -(-129 // c)
        return W, 1 << (c - 1), 0, 1 << (c * W - 1)
    W = -(-253 // c)
    return W, 1 << (c - 1), c * W - 253, 1 << 252


def recode(s, c, W):
    """The unique digits with s = sum d_j 2^(cj), d_j in [-2^(c-1), 2^(c-1)) below the top and an unsigned top digit."""
    out = []
    for _ in range(W - 1):
        d = s % (1 << c)
        if d >= 1 << (c - 1):
            d -= 1 << c
        out.append(d)
        s = (s - d) >> c
    return out + [s]


# ---- points with known logarithms -------------------------------------------------------------------------------------------------
_POINTS = {}


def points():
    """(logs, points): 64 points k * G, 32 random k and their r - k, so that P and -P both occur (log p ^ 1 is -log p)"""
    if not _POINTS:
        prng = random.Random(0x6D736D)
        logs, pts = [], []
        for _ in range(32):
            k = prng.randrange(1, R)
            p = o.mul(o.G, k)
            logs += [k, R - k]
            pts += [p, o.neg(p)]
        assert o.mul(o.G, logs[1]) == pts[1] and o.add(pts[0], pts[1]) == o.IDENTITY
        _POINTS["v"] = (logs, pts, pt_arr(pts))
    return _POINTS["v"]


_MUL = {}


def mul_g(k):
    k %= R
    if k not in _MUL:
        _MUL[k] = o.mul(o.G, k)
    return _MUL[k]


# ---- MSM case groups ------------------------------------------------------------------------------------------------------------
def crafted_scalars(c, short, prng):
    """[(class, scalar)] for one (width, shape), built from digit vectors; all within the shape's bound"""
    W, B, s, bound = shape(c, short)
    lo, hi, top = -(1 << (c - 1)), (1 << (c - 1)) - 1, c * (W - 1)
    t_max = bound >> top                       # the largest top digit: reached only under a carry
    out = [("small", 0), ("small", 1), ("all_bits_set", bound - 1)]
    if not short:
        out.append(("r_minus_1", R - 1))
    out += [("digits_most_negative", from_digits([lo] * (W - 1) + [t], c)) for t in (1, t_max)]
    out += [("digits_most_positive", from_digits([hi] * (W - 1) + [t], c)) for t in (0, t_max - 1)]
    for j in range(W - 1):
        out += [("one_digit_unit", 1 << (c * j)), ("one_digit_high_extreme", hi << (c * j)),
                ("one_digit_low_extreme", (1 << (c * (j + 1))) + (lo << (c * j)))]             # digit j = lo under a 1
    out += [("one_digit_unit", 1 << top)] if 1 << top < bound else []      # (a top digit that only a carry reaches: below)
    out += [("largest_top_digit", (t_max << top) + (lo << (c * (W - 2))))]
    out += [("random", prng.randrange(min(R, bound))) for _ in range(200)]
    for cls, x in out:
        assert 0 <= x < bound, (c, short, cls)
    # the generator's own claims, checked with the textbook digits
    ds = {cls: [recode(x, c, W) for k, x in out if k == cls] for cls in {k for k, _ in out}}
    assert all(d[:-1] == [lo] * (W - 1) for d in ds["digits_most_negative"]) and all(d[:-1] == [hi] * (W - 1) for d in ds["digits_most_positive"])
    assert recode(bound - 1, c, W) == [-1] + [0] * (W - 2) + [t_max]                 # the carry runs through every window
    assert max(d[-1] for v in ds.values() for d in v) == t_max and ds["largest_top_digit"][0][-1] == t_max
    for j in range(W - 1):
        assert any(d[j] == lo for d in ds["one_digit_low_extreme"]) and any(d[j] == hi and sum(1 for x in d if x) == 1 for d in ds["one_digit_high_extreme"])
    return out


def group(name, n_kinds, neg_kinds, pidx, scalars, classes):
    N = len(scalars)
    assert N % n_kinds == 0 and len(pidx) == N
    return {"name": name, "n": N // n_kinds, "n_kinds": n_kinds, "neg_kinds": neg_kinds, "pidx": np.array(pidx, np.int64),
            "scalars": list(scalars), "classes": classes}


def msm_groups(c, short):
    """The case groups of one (width, shape): one call of the MSM each.  Counts every class under (c, short, class)."""
    W, B, s, bound = shape(c, short)
    prng = random.Random(0xC0DE00 + 2 * c + int(short))
    lo, hi, top = -(1 << (c - 1)), (1 << (c - 1)) - 1, c * (W - 1)
    crafted = crafted_scalars(c, short, prng)
    groups = []

    def tally(classes):
        for cls in classes:
            count((c, short, cls))

    # "scalars": every top digit under every residue of the term index (full shape: every slot of the top window), then the
    # crafted scalars, each on a point and on its negative
    sc, cls, pidx = [], [], []
    if not short:
        t_max = bound >> top
        for d in range(t_max + 1):
            while True:
                low = [prng.randint(-hi, hi) for _ in range(W - 1)]
                x = from_digits(low + [d], c)
                if 0 <= x < bound:
                    break
            sc += [x] * (1 << s)                        # term index d * 2^s + m: every residue m
            cls += ["top_every_slot"] * (1 << s)
        pidx = [(7 * t + t // 64) % 64 for t in range(len(sc))]
        # (the largest top digit, t_max, needs the carry out of a negative digit below it: drawn above until it fits)
    for i, (k, x) in enumerate(crafted):
        sc += [x, x]
        cls += [k, k]
        pidx += [2 * i % 64, (2 * i + 1) % 64]
    groups.append(group("scalars", 1, 0, pidx, sc, cls))

    # "buckets": many terms in one bucket, and points that meet their negatives or themselves there
    sc, cls, pidx = [], [], []
    for i in range(300):                                # one point, digit 1 = 5 in every scalar, the other digits differ
        ds = [prng.randint(1, hi) for _ in range(W - 1)] + [0]
        ds[1] = 5
        sc.append(from_digits(ds, c)); pidx.append(2); cls.append("same_point_300_one_bucket")
    for i in range(10):                                 # P and -P under one scalar: every bucket of theirs sums to O
        x = prng.randrange(min(R, bound))
        sc += [x, x]; pidx += [2 * i, 2 * i + 1]; cls += ["p_and_minus_p_equal_digits"] * 2
    for i, d in enumerate((1, 5, hi, 2, hi - 1)):       # P with digit d and -P with digit -d in window j: P + P in one bucket
        j = i % (W - 1)
        sc += [d << (c * j), (1 << (c * (j + 1))) - (d << (c * j))]
        assert recode(sc[-1], c, W)[j] == -d
        pidx += [2 * i + 20, 2 * i + 21]; cls += ["p_digit_d_minus_p_digit_minus_d"] * 2
    x = prng.randrange(min(R, bound))
    sc += [x] * 5000; pidx += [t % 64 for t in range(5000)]; cls += ["shared_scalar_5000"] * 5000
    groups.append(group("buckets", 1, 0, pidx, sc, cls))

    # sizes and kinds: the crafted scalars, then random ones
    pool = [x for _, x in crafted]

    def take(N, start):
        return [pool[(start + t) % len(pool)] if t < len(pool) else prng.randrange(min(R, bound)) for t in range(N)]

    for i, N in enumerate((1, 63, 64, 65, 257, 4097)):
        groups.append(group("n=%d" % N, 1, 0, [(t * 5 + i) % 64 for t in range(N)], take(N, 3 * i + 2), ["n=%d" % N]))
    for i, (kinds, negs, n) in enumerate(((2, 0b01, 131), (4, 0b0101, 67), (3, 0b001, 101), (1, 0b1, 259), (2, 0b11, 77))):
        assert n & (n - 1)
        name = "kinds %d/0b%s" % (kinds, format(negs, "0%db" % kinds))
        groups.append(group(name, kinds, negs, [(t * 3 + i) % 64 for t in range(kinds * n)], take(kinds * n, 11 * i), [name]))
    for g in groups:
        tally(set(g["classes"]))
    return groups


def msm_reference(g, c, short):
    """What the stages must leave for group g: off (W * B + 1), the sorted entries as (bucket, entry) in canonical order, the
    window sums and the total as affine points -- from the textbook digits, Python integers and one o.mul per sum."""
    W, B, s, bound = shape(c, short)
    logs, _, _ = points()
    N, n = len(g["scalars"]), g["n"]
    cache = {}
    for x in g["scalars"]:
        if x not in cache:
            assert 0 <= x < bound
            cache[x] = recode(x, c, W)
    D = np.array([cache[x] for x in g["scalars"]], np.int64)                          # (N, W)
    t = np.arange(N, dtype=np.int64)
    neg = ((g["neg_kinds"] >> (t // n)) & 1).astype(bool)
    ids, entries = [], []
    for j in range(W):
        d = D[:, j]
        nz = d != 0
        mag = np.abs(d[nz]) - 1
        slot = mag if j < W - 1 else (mag << s) | (t[nz] & ((1 << s) - 1))
        assert (slot < B).all() and (j < W - 1 or (d[nz] > 0).all()), (c, short, j)          # the contract of the scalars' bound
        ids.append(j * B + slot)
        entries.append(t[nz] | np.where((d[nz] < 0) != neg[nz], MSM_NEG, 0))
    ids, entries = np.concatenate(ids), np.concatenate(entries)
    counts = np.bincount(ids, minlength=W * B)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    order = np.lexsort((entries, ids))
    # the sums: per point, the signed digits and the signed scalars added as integers, then one multiple of G each
    Ds = np.where(neg[:, None], -D, D)
    win_k, total_k = [0] * W, 0
    for p in range(64):
        sel = g["pidx"] == p
        if not sel.any():
            continue
        col = Ds[sel].sum(axis=0)
        for j in range(W):
            win_k[j] += int(col[j]) * logs[p]
        total_k += sum(-g["scalars"][i] if neg[i] else g["scalars"][i] for i in np.nonzero(sel)[0]) * logs[p]
    assert (sum(k << (c * j) for j, k in enumerate(win_k)) - total_k) % R == 0                  # the digits add up to the scalars
    return {"off": off, "ids": ids[order], "entries": entries[order].astype(np.uint32), "counts": counts,
            "win": [mul_g(k) for k in win_k], "total": mul_g(total_k), "win_k": win_k, "total_k": total_k}


def msm_inputs(g):
    """(points (N, 64), scalars (N, 32)) of group g"""
    _, _, arr = points()
    return np.ascontiguousarray(arr[g["pidx"]]), fe_arr(g["scalars"])


def check_msm(ref, off, order, win, total, what, point_eq):
    """off, order: uint32 arrays; win: W points, total: one point, in whatever form point_eq(got, want, what) compares.  All exact;
    the order within a bucket is free."""
    assert len(off) == len(ref["off"]) and (off == ref["off"]).all(), (what, "off")
    assert len(order) == int(ref["off"][-1]), (what, "order length")
    bucket = np.repeat(np.arange(len(ref["counts"]), dtype=np.int64), ref["counts"])
    got = order[np.lexsort((order, bucket))]
    assert (got == ref["entries"]).all(), (what, "order", int(np.nonzero(got != ref["entries"])[0][0]))
    for j, want in enumerate(ref["win"]):
        point_eq(win[j], want, (what, "window", j))
    point_eq(total, ref["total"], (what, "total"))


def check_top_slots(c, ref):
    """the full shape's "scalars" group fills slots 0 and B - 1 of every window and every slot of the top window"""
    W, B, s, _ = shape(c, False)
    cnt = ref["counts"].reshape(W, B)
    assert (cnt[:, 0] > 0).all() and (cnt[:, B - 1] > 0).all() and (cnt[W - 1] > 0).all() and cnt[W - 1, B - 1] > 0, c


def check_end_slots(c, short, ref):
    W, B, _, _ = shape(c, short)
    cnt = ref["counts"].reshape(W, B)
    assert (cnt[:, 0] > 0).all() and (cnt[:, B - 1] > 0).all(), (c, short)


def point_eq_limbs(got, want, what):
    check_point(got, want, what)


def assert_msm_classes():
    for c, short in SHAPES:
        for cls in MSM_CLASSES + (() if short else FULL_ONLY_CLASSES):
            assert CLASS_COUNTS.get((c, short, cls), 0) > 0, (c, short, cls)


# ---- key-set cases ----------------------------------------------------------------------------------------------------------------
KEYSET_SETS = [(scheme, nk) for scheme in ("single", "double") for nk in (64, 65, 300)]
KEYSET_NS = (1, 511, 512, 513, 1300, 2100)
KEYSET_CLASSES = ("all_first_key", "all_last_key", "boundary_on_line", "boundary_before_line", "boundary_after_line", "run_across_four_lines",
                  "empty_runs_between_full", "runs_of_one", "random", "zero_sum_run", "identity_key_summed", "a=0", "a=1", "a=r-1", "a=random",
                  "run_longer_than_512")


def keyset_keys(scheme, nk):
    """(logs per point column, key columns): k * G with known k; key nk // 2 of column 0 is the identity (log 0, registered as
    not valid: it has no tables)"""
    prng = random.Random(0x6B7300 + nk + (1000 if scheme == "double" else 0))
    cols = 1 if scheme == "single" else 2
    base = [prng.randrange(1, R) for _ in range(cols)]
    logs, keys = [None] * cols, []
    for ci in range(cols):                                  # k_i = base + i (a chain of additions instead of nk multiplications)
        logs[ci] = [0 if (ci == 0 and i == nk // 2) else (base[ci] + i) % R for i in range(nk)]
        p, pts = o.mul(o.G, base[ci]), []
        for i in range(nk):
            pts.append(o.IDENTITY if logs[ci][i] == 0 else p)
            p = o.add(p, o.G)
        assert pts[-1] == o.mul(o.G, logs[ci][-1])
        keys.append(pt_arr(pts))
    return logs, keys


def _runs_to_idx(runs, n):
    """runs: [(key, length)] in key order -> n indices"""
    idx = [k for k, length in runs for _ in range(length)]
    assert len(idx) == n, (len(idx), n)
    return idx


def index_patterns(n, nk, prng):
    """[(class, key indices in key order)]: where the runs of the keys start and end against the lines at multiples of 512"""
    out = [("all_first_key", [0] * n), ("all_last_key", [nk - 1] * n)]

    def cut(first):
        runs, k, left = [], 0, n
        for length in [first] + [KSV_PIECE] * (n // KSV_PIECE + 1):
            length = min(length, left)
            if length <= 0:
                break
            runs.append((min(k, nk - 1), length)); k += 3; left -= length
        return _runs_to_idx(runs, n)

    out += [("boundary_on_line", cut(KSV_PIECE)), ("boundary_before_line", cut(KSV_PIECE - 1)), ("boundary_after_line", cut(KSV_PIECE + 1))]
    if n > 100:
        head = min(100, n - 1)
        lines = (n - 1) // KSV_PIECE - head // KSV_PIECE
        out.append(("run_across_four_lines" if lines == 4 else "run_across_%d_lines" % lines, _runs_to_idx([(1, head), (nk - 2, n - head)], n)))
    used = list(range(0, nk, 3))
    out.append(("empty_runs_between_full", sorted(used[i % len(used)] for i in range(n))))
    ones = min(n, nk - 1)
    out.append(("runs_of_one", list(range(ones)) + [nk - 1] * (n - ones)))
    out.append(("random", sorted(prng.randrange(nk) for _ in range(n))))
    return out


def keyset_cases(scheme, nk):
    """[case]: idx (n,) uint32 in the caller's (shuffled) order, a (point columns x n integers), expected sums (point columns x
    nk integers) and the expected point.  Counts every class under (scheme, nk, class)."""
    logs, _ = keyset_keys(scheme, nk)
    cols = len(logs)
    prng = random.Random(0x6B7311 + nk + cols)
    cases = []
    for n in KEYSET_NS:
        for cls, idx in index_patterns(n, nk, prng):
            perm = list(range(n))
            prng.shuffle(perm)
            idx = [idx[p] for p in perm]
            a = []
            for ci in range(cols):
                col = []
                for i in range(n):
                    kind = prng.randrange(4)
                    col.append((0, 1, R - 1, prng.randrange(R))[kind])
                    count((scheme, nk, ("a=0", "a=1", "a=r-1", "a=random")[kind]))
                # one run whose sum is 0 mod r (the skip branch): its last item takes minus the sum of the others
                by_key = {}
                for i, k in enumerate(idx):
                    by_key.setdefault(k, []).append(i)
                keys_used = sorted(by_key)
                k0 = keys_used[(ci + len(keys_used) // 3) % len(keys_used)]
                items = by_key[k0]
                col[items[-1]] = -sum(col[i] for i in items[:-1]) % R
                a.append(col)
            sums = [[0] * nk for _ in range(cols)]
            for ci in range(cols):
                for i, k in enumerate(idx):
                    sums[ci][k] = (sums[ci][k] + a[ci][i]) % R
            run_len = np.bincount(idx, minlength=nk)
            assert any(sums[0][k] == 0 and run_len[k] for k in range(nk))
            count((scheme, nk, "zero_sum_run"))
            count((scheme, nk, cls))
            count((scheme, nk, "identity_key_summed"), int(run_len[nk // 2] > 0 and sums[0][nk // 2] != 0))
            count((scheme, nk, "run_longer_than_512"), int(run_len.max() > KSV_PIECE))
            # the point: o.mul / o.add over the keys with S_k != 0, the keys being multiples of G: one multiple of G
            total_k = sum(sums[ci][k] * logs[ci][k] for ci in range(cols) for k in range(nk))
            cases.append({"name": "%s nk=%d n=%d %s" % (scheme, nk, n, cls), "n": n, "idx": np.array(idx, np.uint32),
                          "a": [fe_arr(col) for col in a], "sums": sums, "point": mul_g(total_k), "total_k": total_k})
    return cases


def check_keyset(case, sums, point, what, point_eq):
    """sums: (point columns, nk, 32) bytes; point in the form point_eq compares.  Exact."""
    for ci, col in enumerate(case["sums"]):
        got = [int.from_bytes(sums[ci][k].tobytes(), "little") for k in range(len(col))]
        assert got == col, (what, "S_k", ci, next(k for k in range(len(col)) if got[k] != col[k]))
    point_eq(point, case["point"], (what, "point"))


def assert_keyset_classes():
    for scheme, nk in KEYSET_SETS:
        for cls in KEYSET_CLASSES:
            assert CLASS_COUNTS.get((scheme, nk, cls), 0) > 0, (scheme, nk, cls)

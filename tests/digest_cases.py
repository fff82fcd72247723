"""The cases of jjs_digest / jjs_digest_dev (csrc/digest.h), shared by the CPU build's tests and the GPU's.  A case is a dict:
in (n_el, w) uint8, offsets (n + 1 uint32, or None for a uniform call), k, n, fmt (0 canonical, 1 wide), want (n, 32) the
untruncated digests with zero rows for malformed items, status (n,).  Expected values come from oracle/jjs_oracle_c.py
poseidon_any, called once per length group (its SAFE tag comes from the Python oracle); wide elements are reduced with Python
integers first.  Every expected value is computed once per process."""
import functools

import numpy as np

import jjs_oracle as o
import jjs_oracle_c as oc

Q = o.Q
MASK250 = (1 << 250) - 1
BLOCK_EDGE = (1, 3, 4, 5, 8, 9)          # the sponge's rate is 4
CONST_TABLE_EDGE = (16, 17)              # JJS_SPONGE_TAG covers 16 inputs
LONG_TABLE_EDGE = (1027, 1028, 1031)     # JJS_SPONGE_TAG_LONG covers 1027: 1028 is the first tag computed on the device
LENGTHS = BLOCK_EDGE + CONST_TABLE_EDGE + LONG_TABLE_EDGE
SIZES = (1, 63, 64, 65, 257)
RANGE_BAD = (Q, Q + 1, (1 << 256) - 1)
RANGE_GOOD = (Q - 1, 0)
WIDE_EDGES = (0, Q, 2 * Q, 1 << 256, (1 << 512) - 1, ((Q - 1) << 256) + (Q - 1))


def le(x: int, width: int = 32) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(width, "little"), np.uint8).copy()


def to_int(row) -> int:
    return int.from_bytes(bytes(row), "little")


def rand_canonical(rng, count: int) -> np.ndarray:
    return np.stack([le(int.from_bytes(rng.bytes(40), "little") % Q) for _ in range(count)]) if count else np.zeros((0, 32), np.uint8)


def truncated(want: np.ndarray) -> np.ndarray:
    """digest_truncated: the low 250 bits"""
    t = want.copy()
    t[:, 31] &= 0x03
    return t


def expected(values: np.ndarray, offsets) -> np.ndarray:
    """(n, 32) untruncated digests of the items of canonical `values` (n_el, 32): one poseidon_any call per distinct length"""
    n = len(offsets) - 1
    lens = np.diff(np.asarray(offsets, np.int64))
    out = np.zeros((n, 32), np.uint8)
    for k in np.unique(lens):
        idx = np.where(lens == k)[0]
        rows = np.stack([values[offsets[i]:offsets[i] + k] for i in idx])
        out[idx] = oc.poseidon_any(rows)
    return out


def python_digest(values: np.ndarray, offsets, i: int) -> np.ndarray:
    return le(o.poseidon_digest([to_int(r) for r in values[offsets[i]:offsets[i + 1]]]))


def _case(inp, offsets, k, n, fmt, values, status=None):
    """values: the canonical value of every element (what the oracle hashes); status: None = all 0"""
    offs = np.asarray(offsets if offsets is not None else np.arange(n + 1, dtype=np.int64) * k, np.int64)
    want = expected(values, offs)
    status = np.zeros(n, np.uint8) if status is None else status
    want[status == 3] = 0
    return {"in": inp, "offsets": None if offsets is None else np.asarray(offsets, np.uint32), "k": k, "n": n, "fmt": fmt, "want": want,
            "status": status, "values": values, "offs": offs}


@functools.lru_cache(maxsize=None)
def uniform(k: int, n: int):
    """n items of k random canonical elements"""
    rng = np.random.default_rng(1000 * k + n)
    v = rand_canonical(rng, k * n)
    return _case(v, None, k, n, 0, v)


def ragged_lengths(n: int = 200):
    lens = [1 + (37 * i % 131) for i in range(n)]
    lens[7] = 1031
    return lens


@functools.lru_cache(maxsize=None)
def ragged(reverse: bool = False):
    lens = ragged_lengths()
    if reverse:
        lens = lens[::-1]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    rng = np.random.default_rng(7 + reverse)
    v = rand_canonical(rng, int(offsets[-1]))
    return _case(v, offsets, 0, len(lens), 0, v)


def as_offsets(case):
    """a uniform case given through offsets: must equal the uniform call byte for byte"""
    c = dict(case)
    c["offsets"] = (np.arange(case["n"] + 1, dtype=np.int64) * case["k"]).astype(np.uint32)
    c["k"] = 0
    return c


@functools.lru_cache(maxsize=None)
def range_test():
    """Items of length 1, 5 and 9 with q, q + 1, 2^256 - 1 (status 3) and q - 1, 0 (status 0) at element 0, 3, 4 and last, each
    between two good neighbours: 3 items per probe, so that bad and good items share waves and eight-lane groups."""
    rng = np.random.default_rng(31)
    rows, offsets, status = [], [0], []
    for length in (1, 5, 9):
        for pos in sorted({p for p in (0, 3, 4, length - 1) if p < length}):
            for x in RANGE_BAD + RANGE_GOOD:
                for role in ("left", "probe", "right"):
                    item = rand_canonical(rng, length)
                    if role == "probe":
                        item[pos] = le(x)
                    rows.append(item)
                    offsets.append(offsets[-1] + length)
                    status.append(3 if role == "probe" and x >= Q else 0)
    inp = np.concatenate(rows)
    status = np.array(status, np.uint8)
    values = inp.copy()
    for i in np.where(status == 3)[0]:                      # the oracle is not asked about a malformed item
        values[offsets[i]:offsets[i + 1]] = 0
    return _case(inp, np.array(offsets, np.uint32), 0, len(status), 0, values, status)


@functools.lru_cache(maxsize=None)
def wide():
    """Wide elements: the edges and random 512-bit values, in items of length 1, 4 and 5"""
    rng = np.random.default_rng(41)
    ints, offsets = [], [0]
    for length in (1, 4, 5):
        for x in WIDE_EDGES:
            for pos in sorted({0, length - 1}):
                item = [int.from_bytes(rng.bytes(64), "little") for _ in range(length)]
                item[pos] = x
                ints += item
                offsets.append(offsets[-1] + length)
        for _ in range(24):
            ints += [int.from_bytes(rng.bytes(64), "little") for _ in range(length)]
            offsets.append(offsets[-1] + length)
    inp = np.stack([le(x, 64) for x in ints])
    values = np.stack([le(x % Q) for x in ints])
    return _case(inp, np.array(offsets, np.uint32), 0, len(offsets) - 1, 1, values)


def block_order(offsets) -> np.ndarray:
    """the items by ceil(len / 4), descending and stable: restated with numpy"""
    blocks = (np.diff(np.asarray(offsets, np.int64)) + 3) // 4
    return np.argsort(-blocks, kind="stable").astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _filler(count: int):
    """`count` items of one random canonical element each, with their digests"""
    rng = np.random.default_rng(500 + count)
    v = rand_canonical(rng, count)
    return v, oc.poseidon_any(v.reshape(count, 1, 32))


def padded(case, n: int):
    """`case` followed by items of one element up to n items, as a ragged call: how a small case reaches the route of large calls"""
    extra = n - case["n"]
    assert extra >= 0
    if extra == 0 and case["offsets"] is not None:
        return case
    w = case["in"].shape[1]
    v, d = _filler(extra) if extra else (np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
    fill = v if w == 32 else np.concatenate([v, np.zeros_like(v)], axis=1)
    offs = np.concatenate([case["offs"], case["offs"][-1] + 1 + np.arange(extra, dtype=np.int64)])
    return {"in": np.concatenate([case["in"], fill]), "offsets": offs.astype(np.uint32), "k": 0, "n": n, "fmt": case["fmt"],
            "want": np.concatenate([case["want"], d]), "status": np.concatenate([case["status"], np.zeros(extra, np.uint8)]),
            "values": np.concatenate([case["values"], v]), "offs": offs}


@functools.lru_cache(maxsize=None)
def every_length():
    """one ragged call with every length of LENGTHS, three items each, long and short interleaved"""
    lens = [k for _ in range(3) for k in LENGTHS]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    v = rand_canonical(np.random.default_rng(77), int(offsets[-1]))
    return _case(v, offsets, 0, len(lens), 0, v)


@functools.lru_cache(maxsize=None)
def uniform_tiled(k: int, n: int, distinct: int = 48):
    """n items of k elements that repeat `distinct` random items in turn: a long uniform call whose expected values cost `distinct`
    digests (the kernels know nothing of the repetition)"""
    base = uniform(k, distinct)
    idx = np.arange(n) % distinct
    v = base["in"].reshape(distinct, k, 32)[idx].reshape(n * k, 32)
    return {"in": v, "offsets": None, "k": k, "n": n, "fmt": 0, "want": base["want"][idx], "status": np.zeros(n, np.uint8), "values": v,
            "offs": np.arange(n + 1, dtype=np.int64) * k}

"""Cases and expectations of the per-item passes of the two verdict algorithms under the pinned seed, shared by
the CPU build (test_fr_host.py) and the device (fr_items_child.py): what bv_item / ksv_item write for every item -- z on R,
z c mod r on PK, z u mod r on Gen or in the sum -- the per-block partial sums of verdict_item_pass, the fail word and the
totals.  z and z' come from the Python ChaCha20 of tests/fr_cases.py, c from the C oracle (oracle_verify(..., want_c=True)),
which items fail from the oracle's statuses (1 and 3 fail, 0 and 2 pass every per-item check); the products and sums are
Python integers.  Every comparison is an equality of bytes."""
import functools

import numpy as np

import fr_cases as frc
import jjs_oracle as o
from helpers import ARG_ORDER, IDENT, _add_order2, fe_bytes, make_batch, oracle_verify, to_int

R, Q = o.R_ORDER, o.Q
SCHEMES = ("single", "double", "vargen")
SCHEME_ID = {"single": 0, "double": 1, "vargen": 2}
WIDTHS = (8, 9, 10, 11, 14, 16)                      # window widths with distinct weight bits: 135, 134, 129, 131, 139, 143
BLOCK = 256                                          # lanes per block of the item kernels
NS = (1, 63, 64, 65, 255, 256, 257, 1300)
FORCED_BLOCKS = (1, 2, 5)                            # at n = 1300: a lane sums up to six items, the last stride is ragged
FAILING = ("u = r", "u = 2^256 - 1", "coordinate = q", "identity key", "torsion component", "R off the curve")
KEYSET_KEYS, KEYSET_NS, KEYSET_BLOCKS = 300, (1, 257, 1300), (0, 2)
CLASS_COUNTS = {}


def count(cls, n=1):
    CLASS_COUNTS[cls] = CLASS_COUNTS.get(cls, 0) + n


def weight_bits(c):
    """msm_weight_bits of csrc/msm.h"""
    return c * ((129 + c - 1) // c) - 1


assert sorted(weight_bits(c) for c in WIDTHS) == sorted(frc.WEIGHT_BITS) == sorted({weight_bits(c) for c in range(8, 17)})


@functools.lru_cache(maxsize=None)
def _block(item):
    return frc.chacha20_block(frc.PINNED_SEED, item & frc.M32, (item >> 32).to_bytes(4, "little") + bytes(8))


def z_of(item, bits):
    blk, mask = _block(item), (1 << bits) - 1
    return int.from_bytes(blk[:20], "little") & mask, int.from_bytes(blk[20:40], "little") & mask


# ---- batches ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _good(scheme, n, seed):
    return make_batch(scheme, n, seed=seed, n_keys=min(n, 40), mix=False)


def good(scheme, n, seed=610):
    return {k: v.copy() for k, v in _good(scheme, n, seed).items()}


def spoil(b, cls, i):
    """item i of batch b made to fail (or, for the chosen u, to keep passing) the per-item checks"""
    if cls == "u = r":
        b["u"][i] = fe_bytes(R)
    elif cls == "u = 2^256 - 1":
        b["u"][i] = 0xFF
    elif cls == "coordinate = q":
        b["PK"][i, :32] = fe_bytes(Q)
    elif cls == "identity key":
        b["PK"][i] = IDENT
    elif cls == "torsion component":
        b["R"][i] = _add_order2(b["R"][i:i + 1])[0]
    elif cls == "R off the curve":
        b["R"][i, 32] ^= 1
    elif cls.startswith("chosen u"):
        b["u"][i] = fe_bytes({"chosen u = 0": 0, "chosen u = 1": 1, "chosen u = r - 1": R - 1}[cls])
    else:
        raise ValueError(cls)


def verdict_cases(scheme):
    """[{name, b, c, blocks, classes}]"""
    out = []
    for i, c in enumerate(WIDTHS):
        out.append({"name": "width %d" % c, "b": good(scheme, 65), "c": c, "blocks": 0, "classes": ["width %d" % c]})
    for i, n in enumerate(NS):
        out.append({"name": "n = %d" % n, "b": good(scheme, n), "c": WIDTHS[i % len(WIDTHS)], "blocks": 0, "classes": ["own grid, n = %d" % n]})
    for i, blocks in enumerate(FORCED_BLOCKS):
        out.append({"name": "n = 1300 in %d blocks" % blocks, "b": good(scheme, 1300), "c": WIDTHS[NS.index(1300) % len(WIDTHS)], "blocks": blocks,
                    "classes": ["forced grid of %d" % blocks]})     # (the batch and the width of "n = 1300": the CPU build runs them once)
    b = good(scheme, 65)
    for j, cls in enumerate(("chosen u = 0", "chosen u = 1", "chosen u = r - 1")):
        for i in (j, 30 + j, 62 + j):
            spoil(b, cls, i)
    out.append({"name": "chosen u, false equations", "b": b, "c": 11, "blocks": 0, "classes": ["chosen u"], "statuses": {0, 2}, "fail": 0})
    for j, cls in enumerate(FAILING):
        b = good(scheme, 65)
        for i in (0, 32, 64):
            spoil(b, cls, i)
        out.append({"name": cls + " at the first, a middle and the last item", "b": b, "c": WIDTHS[j], "blocks": 0, "classes": ["failing: " + cls],
                    "bad": (0, 32, 64), "fail": 1})
    b = good(scheme, 257)
    spoil(b, "u = r", 256)                                  # the only lane of the last wave and block
    out.append({"name": "u = r at the lone item of the last block", "b": b, "c": 8, "blocks": 0, "classes": ["failing: lone lane of the last block"],
                "bad": (256,), "fail": 1})
    return out


def expected(scheme, case, blocks_used, gathered=None):
    """-> dict of the expected bytes.  gathered: the key-set variant (the key columns the device hashes, gathered per item)"""
    b = case["b"]
    n = len(b["u"])
    bits = weight_bits(case["c"])
    hashed = b if gathered is None else dict(b, **gathered)
    status, cs = oracle_verify(scheme, hashed, want_c=True)
    if "statuses" in case:
        assert set(status.tolist()) == case["statuses"], (case["name"], status.tolist())
    for i in case.get("bad", ()):
        assert status[i] in (1, 3), (case["name"], i, status[i])
    ok = [s in (0, 2) for s in status.tolist()]
    assert all(ok[i] for i in range(n) if i not in case.get("bad", ()) and i not in case.get("bad_key_items", ())), case["name"]
    n_eq = 2 if scheme == "double" else 1
    kinds = {e: [] for e in range(n_eq)}                   # per equation: (z, z c) per item
    zu = [[0] * n for _ in range(2)]
    zgen = []
    for i in range(n):
        z = z_of(i, bits)
        c, u = to_int(cs[i]), to_int(b["u"][i])
        for e in range(n_eq):
            w = z[e] if ok[i] else 0
            kinds[e].append((w, w * c % R))
            if scheme == "vargen":
                zgen.append(w * u % R)
            else:
                zu[e][i] = w * u % R
        count("items " + ("passing" if ok[i] else "failing"))
    part = [[0, 0] for _ in range(blocks_used)]
    for i in range(n):
        for e in range(2):
            part[(i // BLOCK) % blocks_used][e] = (part[(i // BLOCK) % blocks_used][e] + zu[e][i]) % R
    le = lambda xs: b"".join(int(x).to_bytes(32, "little") for x in xs)  # noqa: E731
    out = {"partial": b"".join(le(p) for p in part), "zu": le([sum(zu[0]) % R, sum(zu[1]) % R]), "fail": int(not all(ok))}
    if "fail" in case:
        assert out["fail"] == case["fail"], case["name"]
    if gathered is None:
        out["scalars"] = b"".join(le([k[0] for k in kinds[e]]) + le([k[1] for k in kinds[e]]) for e in range(n_eq)) + le(zgen)
    else:
        out["scalars"] = b"".join(le([k[0] for k in kinds[e]]) for e in range(n_eq))
        out["a"] = [le([k[1] for k in kinds[e]]) for e in range(n_eq)]
    for cls in case["classes"]:
        count(cls)
    if max(((i // BLOCK) // blocks_used for i in range(n)), default=0) >= 2:
        count("a lane sums three items or more")
    if n % (BLOCK * blocks_used) not in (0, n) and n > BLOCK * blocks_used:
        count("ragged last stride")
    return out


def grids_of(cases, case):
    """the block counts of the cases that share `case`'s batch and width: the CPU build serves them with one run"""
    same = [x for x in cases if x["c"] == case["c"] and all(np.array_equal(x["b"][k], case["b"][k]) for k in case["b"])]
    return sorted({x["blocks"] or own_grid(len(x["b"]["u"])) for x in same})


def compare(name, want, got, blocks=None):
    """got["partial"]: the bytes, or (the CPU build's) a dict of them by block count, of which `blocks` is compared"""
    partial = got["partial"][blocks] if isinstance(got["partial"], dict) else got["partial"]
    assert bytes(partial) == want["partial"], (name, "partial")
    for key in ("scalars", "zu"):
        assert bytes(got[key]) == want[key], (name, key)
    assert int(got["fail"]) == want["fail"], (name, "fail word", got["fail"])
    for ci, a in enumerate(want.get("a", [])):
        assert bytes(got["a"][ci]) == a, (name, "a%d" % ci)


def batch_columns(scheme, b):
    """the six column slots of jjs_debug_verdict_items_dev / the CPU twin: the columns in ABI order, None for the unused"""
    cols = [b[k] for k in ARG_ORDER[scheme]]
    return cols + [None] * (6 - len(cols))


# ---- the key-set variant -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def keyset(scheme):
    """-> (the registered key columns with key KEYSET_KEYS // 2 of column 0 replaced by the identity, the 1 300-item batch)"""
    b = make_batch(scheme, 1300, seed=611, n_keys=KEYSET_KEYS, mix=False)
    keys = [b["PK"][:KEYSET_KEYS].copy()] + ([b["PKp"][:KEYSET_KEYS].copy()] if scheme == "double" else [])
    keys[0][KEYSET_KEYS // 2] = IDENT
    return keys, b


def keyset_cases(scheme):
    keys, full = keyset(scheme)
    out = []
    for i, n in enumerate(KEYSET_NS):
        for blocks in KEYSET_BLOCKS:
            b = {k: v[:n].copy() for k, v in full.items()}
            classes = ["key set: n = %d, blocks %d" % (n, blocks)]
            if n == 257:
                for j, cls in enumerate(("chosen u = 0", "chosen u = 1", "chosen u = r - 1")):
                    spoil(b, cls, 10 + j)
                spoil(b, "u = r", 256)
                spoil(b, "R off the curve", 64)
                classes += ["key set: chosen u", "key set: failing signature"]
            idx = (np.arange(n) % KEYSET_KEYS).astype(np.uint32)
            bad_key = tuple(int(x) for x in np.where(idx == KEYSET_KEYS // 2)[0])
            if bad_key:
                classes.append("key set: items on the key that is not valid")
            out.append({"name": "%s set, n = %d, blocks %d" % (scheme, n, blocks), "b": b, "idx": idx, "c": WIDTHS[2 * i % len(WIDTHS)],
                        "blocks": blocks, "classes": classes, "bad": (256, 64) if n == 257 else (), "bad_key_items": bad_key,
                        "fail": int(bool(bad_key) or n == 257)})
    return out


def keyset_expected(scheme, case, blocks_used):
    keys, _ = keyset(scheme)
    gathered = {"PK": keys[0][case["idx"]]}
    if scheme == "double":
        gathered["PKp"] = keys[1][case["idx"]]
    want = expected(scheme, case, blocks_used, gathered)
    status = oracle_verify(scheme, dict(case["b"], **gathered))
    for i in case["bad_key_items"]:
        assert status[i] == 1, (case["name"], i)                 # the identity key: InvalidPoint
    return want


def own_grid(n):
    return (n + BLOCK - 1) // BLOCK


def classes_populated(keysets=True):
    need = ["width %d" % c for c in WIDTHS] + ["own grid, n = %d" % n for n in NS] + ["forced grid of %d" % k for k in FORCED_BLOCKS]
    need += ["chosen u", "failing: lone lane of the last block", "items passing", "items failing", "a lane sums three items or more",
             "ragged last stride"] + ["failing: " + c for c in FAILING]
    if keysets:
        need += ["key set: n = %d, blocks %d" % (n, k) for n in KEYSET_NS for k in KEYSET_BLOCKS]
        need += ["key set: chosen u", "key set: failing signature", "key set: items on the key that is not valid"]
    missing = [c for c in need if CLASS_COUNTS.get(c, 0) == 0]
    assert not missing, missing

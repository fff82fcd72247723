"""Key sets by key (csrc/keyset_lookup.h): a Python restatement of the table's hash, the model every lookup is checked
against -- a dict from a key's canonical bytes to the LOWEST index it is registered at -- and the crafted sets shared by
tests/test_keyset_lookup_host.py (CPU build) and tests/keyset_lookup_child.py (device, hash seed pinned to 0).

Lookup needs no valid curve points: most keys here are random canonical coordinates, and keys that collide in the table
are found by brute force over the Python hash."""
import itertools

import numpy as np

import jjs_oracle as o

M64 = (1 << 64) - 1
MISS = 0xFFFFFFFF
EMPTY = 0xFFFFFFFF
FORMATS = {"affine": 0, "ext": 1, "wire": 2}


def slot_count(n_keys: int) -> int:
    s = 8
    while s < 2 * n_keys:
        s <<= 1
    return s


def encoding(pt: bytes) -> bytes:
    """The 32 encoding bytes of a 64-byte affine row: v with bit 255 replaced by the parity of u."""
    v = bytearray(pt[32:64])
    v[31] = (v[31] & 0x7F) | ((pt[0] & 1) << 7)
    return bytes(v)


def kl_hash(row: bytes, seed: int = 0) -> int:
    """row: the key's affine points side by side (64 or 128 bytes)."""
    h = 0x9E3779B97F4A7C15 ^ seed
    for p in range(0, len(row), 64):
        e = encoding(row[p:p + 64])
        for k in range(4):
            h ^= int.from_bytes(e[8 * k:8 * k + 8], "little")
            h = (h * 0xFF51AFD7ED558CCD) & M64
            h ^= h >> 29
    return h


def slot_of(row: bytes, mask: int, seed: int = 0) -> int:
    return (kl_hash(row, seed) & 0xFFFFFFFF) & mask


def rand_row(rng, cols: int) -> bytes:
    """Random canonical coordinates (below 2^254 < q): a key as far as the lookup is concerned."""
    a = bytearray(rng.bytes(64 * cols))
    for i in range(31, 64 * cols, 32):
        a[i] &= 0x3F
    return bytes(a)


def row_for_slot(rng, cols: int, slot: int, mask: int) -> bytes:
    while True:
        r = rand_row(rng, cols)
        if slot_of(r, mask) == slot:
            return r


def row_not_in_slots(rng, cols: int, slots, mask: int) -> bytes:
    while True:
        r = rand_row(rng, cols)
        if slot_of(r, mask) not in slots:
            return r


def _canonical(pt: bytes) -> bool:
    return int.from_bytes(pt[:32], "little") < o.Q and int.from_bytes(pt[32:], "little") < o.Q


def _on_curve(pt: bytes) -> bool:
    return o.is_on_curve((int.from_bytes(pt[:32], "little"), int.from_bytes(pt[32:], "little")))


def model(keys, bad=None):
    """keys: list of rows (64 * cols bytes).  Returns (affine dict, wire dict): canonical bytes -> lowest index."""
    affine, wire = {}, {}
    for i, row in enumerate(keys):
        pts = [row[p:p + 64] for p in range(0, len(row), 64)]
        if (bad is not None and bad[i]) or not all(_canonical(p) for p in pts):
            continue
        affine.setdefault(row, i)
        if all(_on_curve(p) for p in pts):
            wire.setdefault(b"".join(encoding(p) for p in pts), i)
    return affine, wire


def ext_to_affine(pt96: bytes):
    """None for an unusable point (U, V or Z >= q, or Z = 0)."""
    U, V, Z = (int.from_bytes(pt96[k:k + 32], "little") for k in (0, 32, 64))
    if U >= o.Q or V >= o.Q or Z >= o.Q or Z == 0:
        return None
    zi = o.fq_inv(Z)
    return o.le32(U * zi % o.Q) + o.le32(V * zi % o.Q)


def to_ext(pt: bytes, z: int) -> bytes:
    u, v = int.from_bytes(pt[:32], "little"), int.from_bytes(pt[32:], "little")
    return o.le32(u * z % o.Q) + o.le32(v * z % o.Q) + o.le32(z)


def want(keys, fmt, queries, bad=None):
    """queries: rows of the query in `fmt` (affine 64 * cols, ext 96 * cols, wire 32 * cols bytes)."""
    affine, wire = model(keys, bad)
    out = []
    for q in queries:
        if fmt == "wire":
            out.append(wire.get(q, MISS))
        elif fmt == "ext":
            pts = [ext_to_affine(q[p:p + 96]) for p in range(0, len(q), 96)]
            out.append(MISS if any(p is None for p in pts) else affine.get(b"".join(pts), MISS))
        else:
            out.append(affine.get(q, MISS))
    return np.array(out, np.uint32)


def case(name, cols, keys, fmt, queries, bad=None, orders=None, slots=None, expect=None):
    w = want(keys, fmt, queries, bad)
    if expect is not None:       # what the case is ABOUT, stated by hand; the model must agree
        assert w.tolist() == list(expect), (name, w.tolist(), list(expect))
    assert len(keys) <= 64 and len(queries) <= 256, name
    return {"name": name, "cols": cols, "keys": keys, "fmt": fmt, "queries": queries, "bad": bad, "orders": orders, "slots": slots, "want": w}


def curve_point(k: int) -> bytes:
    p = o.mul(o.G, k)
    return o.le32(p[0]) + o.le32(p[1])


IDENT = o.le32(0) + o.le32(1)


def crafted(cols: int):
    """The sets whose layout in the table is chosen (hash seed 0): wrap-around, chains, the all-equal set."""
    rng = np.random.default_rng(1000 + cols)
    out = []
    # three keys on slot 7 of 8: the chain wraps to slots 0 and 1
    ks = [row_for_slot(rng, cols, 7, 7) for _ in range(3)]
    stranger = row_for_slot(rng, cols, 7, 7)         # walks 7, 0, 1 and misses at the empty slot 2
    out.append(case(f"wrap{cols}", cols, ks, "affine", ks + [stranger], slots=[1, 2, None, None, None, None, None, 0], expect=[0, 1, 2, MISS]))
    # 40 keys in 128 slots: five colliders on slot 100 (hits behind 0 .. 4 colliders), a key alone in its slot (first probe),
    # a stranger that walks the whole chain to the empty slot behind it
    mask = 127
    chain = [row_for_slot(rng, cols, 100, mask) for _ in range(5)]
    alone = row_for_slot(rng, cols, 50, mask)
    fill = [row_not_in_slots(rng, cols, set(range(84, 107)) | set(range(34, 52)), mask) for _ in range(34)]     # (and none spills into them)
    ks = fill[:10] + chain + fill[10:] + [alone]
    stranger = row_for_slot(rng, cols, 100, mask)
    out.append(case(f"chain{cols}", cols, ks, "affine", chain + [alone, stranger] + fill[:4],
                    expect=[10, 11, 12, 13, 14, 39, MISS, 0, 1, 2, 3]))
    # all 64 keys equal: one entry, index 0
    k = rand_row(rng, cols)
    sl = [None] * 128
    sl[slot_of(k, 127)] = 0
    out.append(case(f"equal{cols}", cols, [k] * 64, "affine", [k, rand_row(rng, cols)], slots=sl, expect=[0, MISS]))
    return out


def lookup_cases():
    out = []
    for cols in (1, 2):
        rng = np.random.default_rng(7 + cols)
        # the smallest sets: 1 .. 4 keys in 8 slots, 5 in 16
        for nk in (1, 2, 3, 4, 5):
            assert slot_count(nk) == (8 if nk <= 4 else 16)
            ks = [rand_row(rng, cols) for _ in range(nk)]
            out.append(case(f"small{nk}x{cols}", cols, ks, "affine", ks + [rand_row(rng, cols) for _ in range(5)],
                            expect=list(range(nk)) + [MISS] * 5))
        out += crafted(cols)
        # duplicates at indices 2, 5 and 9, entered in every order: the lowest index whatever the order
        ks = [rand_row(rng, cols) for _ in range(12)]
        ks[5] = ks[9] = ks[2]
        rest = [i for i in range(12) if i not in (2, 5, 9)]
        orders = [rest[:4] + [p[0]] + rest[4:7] + [p[1]] + rest[7:] + [p[2]] for p in itertools.permutations((2, 5, 9))]
        orders += [[p[0], p[1], p[2]] + rest for p in itertools.permutations((2, 5, 9))]
        out.append(case(f"dups{cols}", cols, ks, "affine", ks, orders=orders, expect=[0, 1, 2, 3, 4, 2, 6, 7, 8, 2, 10, 11]))
        # queries that differ from a registered key in one bit of each of its 16 (32) words
        ks = [rand_row(rng, cols) for _ in range(9)]
        qs = [ks[4]]
        for wi in range(16 * cols):
            q = bytearray(ks[4])
            bit = (5 * wi + 3) % 32
            q[4 * wi + bit // 8] ^= 1 << (bit % 8)
            qs.append(bytes(q))
        out.append(case(f"onebit{cols}", cols, ks, "affine", qs, expect=[4] + [MISS] * (16 * cols)))
        # a malformed registered key (u = q) never hits; the registered identity does
        ks = [rand_row(rng, cols) for _ in range(6)]
        ks[1] = o.le32(o.Q) + ks[1][32:]
        ks[3] = IDENT * cols
        out.append(case(f"malformed{cols}", cols, ks, "affine", ks, expect=[0, MISS, 2, 3, 4, 5]))
        # extended queries: every registered key at Z != 1 hits; Z = 0 and U >= q miss
        ks = [rand_row(rng, cols) for _ in range(7)]
        zs = [int.from_bytes(rng.bytes(40), "little") % (o.Q - 2) + 2 for _ in range(7 * cols)]
        qs = [b"".join(to_ext(k[64 * c:64 * c + 64], zs[cols * i + c]) for c in range(cols)) for i, k in enumerate(ks)]
        last = 96 * (cols - 1)                 # the unusable point is the LAST of the key: the first alone would hit
        z0 = qs[2][:last + 64] + o.le32(0)
        ubig = qs[3][:last] + o.le32(o.Q + 5) + qs[3][last + 32:]
        zbig = qs[5][:last + 64] + o.le32(o.Q)
        z1 = b"".join(k[64 * c:64 * c + 64] + o.le32(1) for k in [ks[6]] for c in range(cols))
        out.append(case(f"ext{cols}", cols, ks, "ext", qs + [z0, ubig, zbig, z1], expect=list(range(7)) + [MISS, MISS, MISS, 6]))
    # two-point sets: the right first point with another second point, and the two points swapped
    rng = np.random.default_rng(99)
    ks = [rand_row(rng, 2) for _ in range(8)]
    ks.append(ks[1][64:] + ks[1][:64])          # ... unless the swapped pair is registered too
    qs = [ks[0], ks[0][:64] + ks[2][64:], ks[0][64:] + ks[0][:64], ks[3][:64] + ks[3][:64], ks[1][64:] + ks[1][:64]]
    out.append(case("twopoint", 2, ks, "affine", qs, expect=[0, MISS, MISS, MISS, 8]))
    # wire queries, over real points (the on-curve rule needs them)
    for cols in (1, 2):
        pts = [curve_point(3 + 11 * i) for i in range(10)]
        P = pts[0]
        u = int.from_bytes(P[:32], "little")
        trap = o.le32((u + 2) % o.Q if (u + 2) < o.Q else u - 2) + P[32:]      # off the curve, P's v and the parity of P's u
        assert encoding(trap) == encoding(P) and not _on_curve(trap)
        negP = o.le32(o.Q - u) + P[32:]
        two = lambda a, b: a + b if cols == 2 else a  # noqa: E731
        # the trap at index 0, then points that are on the curve, the identity, and -- at index 5 -- the point whose
        # encoding the trap shares (set A has it, set B does not)
        for name, with_p in (("A", True), ("B", False)):
            ks = [two(trap, pts[1]), two(pts[2], pts[3]), two(IDENT, IDENT), two(pts[4], trap), two(pts[5], pts[6])]
            if with_p:
                ks.append(two(P, pts[1]))
            enc = lambda row: b"".join(encoding(row[p:p + 64]) for p in range(0, len(row), 64))  # noqa: E731
            flipped = bytearray(enc(ks[1])); flipped[31] ^= 0x80
            qs = [enc(two(P, pts[1])), enc(ks[1]), bytes(flipped), enc(ks[2]), enc(two(negP, pts[1])), enc(ks[4]), enc(ks[3])]
            exp = [5 if with_p else MISS, 1, MISS, 2, MISS, 4, MISS if cols == 2 else 3]
            out.append(case(f"wire{name}{cols}", cols, ks, "wire", qs, expect=exp))
            # the same keys by their affine bytes: the off-curve keys ARE found
            out.append(case(f"wire{name}{cols}-affine", cols, ks, "affine", ks, expect=list(range(len(ks)))))
    return out


def columns(c):
    """The case's key columns and query columns as numpy arrays: (keys0, keys1 | None), (Q0, Q1 | None)."""
    cols = c["cols"]
    keys = np.frombuffer(b"".join(c["keys"]), np.uint8).reshape(len(c["keys"]), 64 * cols)
    k = [np.ascontiguousarray(keys[:, 64 * i:64 * i + 64]) for i in range(cols)] + [None] * (2 - cols)
    n = len(c["queries"])
    q = np.frombuffer(b"".join(c["queries"]), np.uint8).reshape(n, -1)
    if c["fmt"] == "wire":
        qc = [np.ascontiguousarray(q), None]
    else:
        w = 96 if c["fmt"] == "ext" else 64
        qc = [np.ascontiguousarray(q[:, w * i:w * i + w]) for i in range(cols)] + [None] * (2 - cols)
    return k, qc


# ---- sets of real keys for the device tests (tests/test_keyset_lookup_gpu.py) ---------------------------------------------
def off_curve_twin(pt: bytes) -> bytes:
    """A canonical point off the curve with the encoding of `pt` (its v, the parity of its u)."""
    u = int.from_bytes(pt[:32], "little")
    t = o.le32(u + 2 if u + 2 < o.Q else u - 2) + pt[32:]
    assert encoding(t) == encoding(pt) and not _on_curve(t)
    return t


UNDECODABLE = b"\xff" * 31 + b"\x7f"           # v >= q


def registered_set(honest, nk: int, fmt: str, rng):
    """A set of the first nk keys of `honest` (rows of 64 * cols bytes, distinct valid keys: at least 600, and nk + 64, whose
    last 64 stay out of every set) with, from
    three keys on, a duplicate; from five on the identity and a malformed key; from 64 on an off-curve twin of a key beside
    that key and one without it, another duplicate and -- registered from extended coordinates -- a point with Z = 0.
    Returns (the columns jjs_keyset_create takes in `fmt`, the affine rows the set then holds, their malformed flags)."""
    cols = len(honest[0]) // 64
    rows = list(honest[:nk])
    special = {}                                # index -> what the encoding of its first point is, by format
    if nk >= 3:
        rows[2] = rows[0]
    if nk >= 5:
        rows[3] = IDENT * cols
        rows[4] = o.le32(o.Q) + rows[4][32:]
        special[4] = "malformed"
    if nk >= 64:
        rows[10] = off_curve_twin(honest[500][:64]) + honest[500][64:]
        rows[11] = honest[500]
        rows[20] = rows[7]
        rows[40] = off_curve_twin(honest[501][:64]) + honest[501][64:]
        special[41] = "z0"
    pts = lambda r: [r[p:p + 64] for p in range(0, len(r), 64)]  # noqa: E731
    held, bad, enc = [], [], []
    for i, r in enumerate(rows):
        p = pts(r)
        if fmt == "affine":
            enc.append(r); held.append(r); bad.append(0 if all(_canonical(x) for x in p) else 1)
        elif fmt == "ext":
            if special.get(i) == "malformed":      # U = q as it stands: nothing to rescale
                e = [p[0] + o.le32(1)] + [to_ext(x, 3) for x in p[1:]]
                held.append(r); bad.append(1)
            elif special.get(i) == "z0":           # not a point: the set holds (0, 0), not malformed
                e = [p[0] + o.le32(0)] + [to_ext(x, 5) for x in p[1:]]
                held.append(bytes(64) + r[64:]); bad.append(0)
            else:
                e = [to_ext(x, int.from_bytes(rng.bytes(40), "little") % (o.Q - 1) + 1) for x in p]
                held.append(r); bad.append(0)
            enc.append(b"".join(e))
        else:
            e = [encoding(x) for x in p]
            if special.get(i) == "malformed":
                e[0] = UNDECODABLE
            dec = [x if _canonical(x) and _on_curve(x) else o.decompress(y) for x, y in zip(p, e)]
            dec = [None if special.get(i) == "malformed" and k == 0 else d for k, d in enumerate(dec)]
            if any(d is None for d in dec):
                held.append((IDENT * cols)); bad.append(1)
            else:
                held.append(b"".join(d if isinstance(d, bytes) else o.le32(d[0]) + o.le32(d[1]) for d in dec)); bad.append(0)
            enc.append(b"".join(e))
    a = np.frombuffer(b"".join(enc), np.uint8).reshape(nk, -1)
    if fmt == "wire":
        create = [np.ascontiguousarray(a), None]
    else:
        w = 96 if fmt == "ext" else 64
        create = [np.ascontiguousarray(a[:, w * c:w * c + w]) for c in range(cols)] + [None] * (2 - cols)
    return create, held, bad


def query_pool(honest, held, fmt: str, rng, n: int = 257):
    """n queries in `fmt`: the set's keys by the bytes it holds, keys that are not in it, off-curve twins, and -- extended --
    unusable points.  Returns the query rows (bytes)."""
    cols = len(honest[0]) // 64
    base = []
    for i in range(n):
        kind = i % 4
        if kind in (0, 1):
            base.append(held[(i // 2) % len(held)])
        elif kind == 2:
            base.append(honest[-64 + (i // 4) % 60])             # registered in no set
        else:
            h = held[i % len(held)]
            base.append(off_curve_twin(h[:64]) + h[64:] if _canonical(h[:64]) and _on_curve(h[:64]) else honest[-1])
    out = []
    for i, r in enumerate(base):
        p = [r[k:k + 64] for k in range(0, len(r), 64)]
        if fmt == "affine":
            out.append(r)
        elif fmt == "wire":
            out.append(b"".join(encoding(x) for x in p))
        else:
            e = [x + o.le32(1) if not _canonical(x) else to_ext(x, int.from_bytes(rng.bytes(40), "little") % (o.Q - 1) + 1) for x in p]
            if i % 29 == 7:
                e[-1] = e[-1][:64] + o.le32(0)
            if i % 31 == 9:
                e[-1] = o.le32(o.Q + 1) + e[-1][32:]
            out.append(b"".join(e))
    return out


def query_columns(queries, cols: int, fmt: str):
    q = np.frombuffer(b"".join(queries), np.uint8).reshape(len(queries), -1) if queries else np.zeros((0, {"affine": 64, "ext": 96, "wire": 32}[fmt] * cols), np.uint8)
    if fmt == "wire":
        return [np.ascontiguousarray(q)]
    w = 96 if fmt == "ext" else 64
    return [np.ascontiguousarray(q[:, w * c:w * c + w]) for c in range(cols)]

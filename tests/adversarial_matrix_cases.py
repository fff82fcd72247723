"""The adversarial battery of the device-path matrix (test_adversarial_matrix_host.py, test_adversarial_matrix_gpu.py,
adversarial_matrix_child.py): per scheme the concatenation of helpers.edge_cases, helpers.torsion_grid (reps=2),
scalar_mul_cases.degenerate_batch and two classes built here --

  exact        items whose FULL equation holds, torsion included (verify_all_cases.cofactorless_torsion for every scheme): the
               key carries a component S of order 2, 4 or 8 and R the matching c*S (per-item generator: R = u*S_gen + c*S_pk);
               for double signatures also with the torsion in the second equation alone.  Status 1: no test of the equations
               can tell them from valid items, only the per-point subgroup tests can.
  precedence   two faults in one item: u >= r with an identity point (3), a coordinate >= q with an off-curve R (3), m >= q with
               a point of order 2 (3), a torsion key or a torsion R with a failing equation (1, not 2).

-- with every item's class name, its reference status, and the three input formats.  The reference statuses come from the C
oracle (helpers.oracle_verify) on the un-tiled battery, for the two new classes also item by item from the Python oracle;
never from the host build and never from the device.  Every class is counted per scheme and per format in CLASS_COUNTS, and
assert_class_counts holds every count non-zero, so a change here or in a format cannot silently empty a class.

The wire reference is a model, not a filter: every 32-byte point string of the wire form is decoded with the Python oracle's
`decompress`; an item with an undecodable string has status 3, every other item the C oracle's status on the DECODED points
(an off-curve point's would-be encoding decodes to another point, or to none).  An item whose affine form has a coordinate
>= q cannot be compressed: that column takes one of the undecodable encodings (v >= q, u = 0 with the sign bit, a v with no
square root) in turn, and the item stays in the battery under its class."""
import functools
import time

import numpy as np

import jjs_oracle as o
from helpers import (ARG_ORDER, IDENT, ORDER2, edge_cases, fe_bytes, make_batch, oracle_verify, pt_bytes, py_verify, to_extended,
                     to_int, to_pt, to_wire, torsion_generator, torsion_grid, wire_point_cases)
from scalar_mul_cases import degenerate_batch

SCHEMES = ("single", "double", "vargen")
FORMATS = ("affine", "ext", "wire")
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}
CLASSES = ("edge_cases", "torsion_grid", "degenerate", "exact", "precedence")
# random assignments over all points behind the (PK, R) grid; sized so that the battery of a scheme with two lookups stays
# below 256 items: tiled to 32 768 items every key then repeats 128 times or more and the engine takes the wide windows
GRID_EXTRA = {"single": 0, "double": 16, "vargen": 16}
CLASS_COUNTS = {}            # (scheme, format) -> {class: items}
BUILD_SECONDS = {}           # scheme -> seconds the construction of its battery took in this process
R, Q = o.R_ORDER, o.Q


def point_cols(scheme):
    return KEYCOLS[scheme] + RCOLS[scheme]


def _stack(scheme, rows):
    return {k: np.stack([r[k] for r in rows]) for k in ARG_ORDER[scheme]}


def _rand(rng, mod):
    return int.from_bytes(rng.bytes(40), "little") % (mod - 1) + 1


# ---- exact: the full equation holds with torsion -----------------------------------------------------------------------------
def exact_plans(scheme):
    """[(name, {key column: k})]: the key column carries k * T8 (order 8 / gcd(k, 8))"""
    if scheme == "single":
        return [("pk_order_%d" % (8 // k), {"PK": k}) for k in (4, 2, 1)] + [("pk_order_8_other", {"PK": 3})]
    if scheme == "double":
        return [("both_order_%d" % (8 // k), {"PK": k, "PKp": k}) for k in (4, 2, 1)] + \
               [("second_only_order_%d" % (8 // k), {"PKp": k}) for k in (4, 2, 1)] + \
               [("first_only_order_8", {"PK": 1}), ("both_different", {"PK": 1, "PKp": 6})]
    return [("gen_order_%d" % (8 // k), {"Gen": k}) for k in (4, 2, 1)] + \
           [("pk_order_%d" % (8 // k), {"PK": k}) for k in (4, 1)] + [("gen_and_pk", {"Gen": 1, "PK": 2}), ("gen_and_pk_other", {"Gen": 6, "PK": 5})]


@functools.lru_cache(None)
def exact_batch(scheme, seed=0xE8AC7):
    """-> (batch, [name], [torsion index of R (and R')]).  The nonce is searched as cofactorless_torsion does: R's torsion part
    must be what the challenge (which depends on R) makes of the keys' parts."""
    rng = np.random.default_rng(seed)
    t8 = torsion_generator()
    T = [o.mul(t8, k) if k else o.IDENTITY for k in range(8)]
    rows, names, r_parts = [], [], []
    for name, tors in exact_plans(scheme):
        a = {k: tors.get(k, 0) for k in KEYCOLS[scheme]}
        sk, m = _rand(rng, R), _rand(rng, Q)
        if scheme == "vargen":
            base = o.mul(o.G, _rand(rng, R))                    # the prime-order part of the generator
            gen = o.add(base, T[a["Gen"]])
        else:
            base = gen = o.G
        PK = o.add(o.mul(base, sk), T[a["PK"]])
        PKp = o.add(o.mul(o.G_NUMS, sk), T[a["PKp"]]) if scheme == "double" else None
        found = None
        for _ in range(200):
            k = _rand(rng, R)
            Rb = o.mul(base, k)
            Rpb = o.mul(o.G_NUMS, k) if scheme == "double" else None
            for g in (1, 2, 3, 4, 5, 6, 7, 0):                  # torsion on R first: the clean R is the last resort
                if scheme == "single":
                    part = (g * a["PK"] % 8,)
                    Rr = o.add(Rb, T[part[0]])
                    c = o.challenge_single(Rr, PK, m)
                    ok = (c - g) * a["PK"] % 8 == 0
                elif scheme == "double":
                    part = (g * a["PK"] % 8, g * a["PKp"] % 8)
                    Rr, Rp = o.add(Rb, T[part[0]]), o.add(Rpb, T[part[1]])
                    c = o.challenge_double(Rr, Rp, PK, PKp, m)
                    ok = (c - g) * a["PK"] % 8 == 0 and (c - g) * a["PKp"] % 8 == 0
                else:
                    part = (g,)
                    Rr = o.add(Rb, T[g])
                    c = o.challenge_vargen(Rr, PK, gen, m)
                    u = (k - c * sk) % R
                    ok = (u * a["Gen"] + c * a["PK"]) % 8 == g
                if ok:
                    found = (k, c, Rr, part)
                    break
            if found:
                break
        assert found, (scheme, name)
        k, c, Rr, part = found
        u = (k - c * sk) % R
        assert o.add(o.mul(gen, u), o.mul(PK, c)) == Rr, (scheme, name)        # the FULL equation, torsion included
        row = {"u": fe_bytes(u), "m": fe_bytes(m), "R": pt_bytes(Rr), "PK": pt_bytes(PK)}
        if scheme == "double":
            Rp = o.add(Rpb, T[part[1]])
            assert o.add(o.mul(o.G_NUMS, u), o.mul(PKp, c)) == Rp, (scheme, name)
            row.update(Rp=pt_bytes(Rp), PKp=pt_bytes(PKp))
        if scheme == "vargen":
            row["Gen"] = pt_bytes(gen)
        rows.append(row); names.append(name); r_parts.append(part)
    assert any(any(p) for p in r_parts), scheme                  # at least one R carries torsion itself
    return _stack(scheme, rows), names, r_parts


# ---- precedence: two faults in one item ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def precedence_batch(scheme):
    """-> (batch, [name], [the status the reference's order of checks gives])"""
    base = make_batch(scheme, 1, seed=0x9CE, mix=False)
    assert oracle_verify(scheme, base).tolist() == [0]
    t8 = torsion_generator()
    rows, names, want = [], [], []

    def variant(name, status, **over):
        d = {k: v[0].copy() for k, v in base.items()}
        d.update(over)
        rows.append(d); names.append(name); want.append(status)

    def off_curve(name):
        r = base[name][0].copy(); r[32] ^= 1
        assert not o.is_on_curve(to_pt(r)) and to_pt(r)[1] < Q
        return r

    def non_canonical(name):
        r = base[name][0].copy(); r[:32] = fe_bytes(Q)
        return r

    def with_torsion(name, k):
        return pt_bytes(o.add(to_pt(base[name][0]), o.mul(t8, k)))

    bad_u = fe_bytes((to_int(base["u"][0]) + 1) % R)
    for name in point_cols(scheme):
        variant("u_ge_r_identity_" + name, 3, u=fe_bytes(R), **{name: IDENT})
        if name == "R":                                          # both faults on R itself: u = q and v off the curve
            r = non_canonical("R"); r[32] ^= 1
            variant("coordinate_ge_q_off_curve_R", 3, R=r)
        else:
            variant("coordinate_ge_q_%s_off_curve_R" % name, 3, **{name: non_canonical(name), "R": off_curve("R")})
        variant("m_ge_q_order2_" + name, 3, m=fe_bytes(Q), **{name: ORDER2})
    for name in KEYCOLS[scheme]:
        for k in (1, 2, 4):
            variant("torsion_key_%s_order_%d_failing_equation" % (name, 8 // k), 1, u=bad_u, **{name: with_torsion(name, k)})
    for name in RCOLS[scheme]:
        for k in (1, 2, 4):
            variant("torsion_%s_order_%d_failing_equation" % (name, 8 // k), 1, u=bad_u, **{name: with_torsion(name, k)})
    return _stack(scheme, rows), names, want


# ---- the battery ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def battery(scheme):
    """-> (batch dict of read-only arrays, (class name per item))"""
    t0 = time.perf_counter()
    parts = [("edge_cases", edge_cases(scheme)), ("torsion_grid", torsion_grid(scheme, reps=2, extra=GRID_EXTRA[scheme])),
             ("degenerate", degenerate_batch(scheme)), ("exact", exact_batch(scheme)[0]), ("precedence", precedence_batch(scheme)[0])]
    b = {k: np.ascontiguousarray(np.concatenate([p[k] for _, p in parts])) for k in ARG_ORDER[scheme]}
    classes = tuple(cls for cls, p in parts for _ in range(len(p["u"])))
    for a in b.values():
        a.setflags(write=False)
    BUILD_SECONDS[scheme] = time.perf_counter() - t0
    return b, classes


def class_rows(scheme, *classes):
    """the positions of the battery's items of these classes"""
    return np.array([i for i, c in enumerate(battery(scheme)[1]) if c in classes])


def subset(b, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in b.items()}


def concat(*bs):
    return {k: np.ascontiguousarray(np.concatenate([b[k] for b in bs])) for k in bs[0]}


def non_canonical_rows(col):
    """rows of a point column with a coordinate >= q"""
    out = np.zeros(len(col), bool)
    for half in (col[:, :32], col[:, 32:]):
        for i in np.where(half[:, 31] >= 0x73)[0]:               # q = 0x73ed...: nothing below is >= q
            out[i] = out[i] or to_int(half[i]) >= Q
    return out


# ---- formats ----------------------------------------------------------------------------------------------------------------------
def undecodable_encodings():
    """The first encoding of each undecodable kind among helpers.wire_point_cases: v >= q, u = 0 with the sign bit, a v with no
    square root."""
    kinds = {}
    for e in wire_point_cases(np.random.default_rng(0), n_random=0):
        if o.decompress(e) is not None:
            continue
        v = int.from_bytes(e, "little") & ((1 << 255) - 1)
        plain = o.decompress(v.to_bytes(32, "little")) if v < Q else None
        kind = "v_ge_q" if v >= Q else ("zero_u_with_sign" if plain is not None and plain[0] == 0 else "non_residue")
        assert kind != "non_residue" or plain is None
        kinds.setdefault(kind, e)
    assert sorted(kinds) == ["non_residue", "v_ge_q", "zero_u_with_sign"]
    return [np.frombuffer(kinds[k], np.uint8) for k in ("v_ge_q", "zero_u_with_sign", "non_residue")]


def wire_columns(scheme, b):
    """{point column: (n, 32) encodings}: helpers.to_wire's, with an undecodable encoding where the affine point has a
    coordinate >= q"""
    big = {k: non_canonical_rows(b[k]) for k in point_cols(scheme)}
    safe = {k: v.copy() for k, v in b.items()}
    for k, rows in big.items():
        safe[k][rows] = pt_bytes(o.G)                            # a placeholder that compresses; overwritten below
    sig, pk, _ = to_wire(scheme, safe)
    cols = {name: sig[:, 32 + 32 * i:64 + 32 * i].copy() for i, name in enumerate(RCOLS[scheme])}
    cols.update({name: pk[:, 32 * i:32 * i + 32].copy() for i, name in enumerate(KEYCOLS[scheme])})
    bad_enc, turn = undecodable_encodings(), 0
    for k in point_cols(scheme):
        for i in np.where(big[k])[0]:
            cols[k][i] = bad_enc[turn % 3]; turn += 1
    return cols


def decode_columns(cols):
    """The wire model: every 32-byte string through the Python oracle's decompress.  -> ({column: (n, 64) affine, G where
    nothing decodes}, {column: undecodable flags})"""
    dec, bad = {}, {}
    memo = {}
    for k, enc in cols.items():
        dec[k], bad[k] = np.empty((len(enc), 64), np.uint8), np.zeros(len(enc), bool)
        for i, e in enumerate(enc):
            key = e.tobytes()
            if key not in memo:
                memo[key] = o.decompress(key)
            p = memo[key]
            bad[k][i] = p is None
            dec[k][i] = pt_bytes(p if p is not None else o.G)
    return dec, bad


class Forms:
    """One batch in its three formats with the reference statuses of every (key format, signature format) pair."""

    def __init__(self, scheme, b, seed=0xF0):
        self.scheme, self.affine = scheme, b
        self.n = len(b["u"])
        rng = np.random.default_rng(seed)
        self.ext = {}
        for k in point_cols(scheme):
            e = to_extended(np.where(non_canonical_rows(b[k])[:, None], pt_bytes(o.G)[None], b[k]), rng)
            big = non_canonical_rows(b[k])                       # nothing to rescale: verbatim with Z = 1
            e[big, :64] = b[k][big]; e[big, 64:] = fe_bytes(1)
            self.ext[k] = e
        self.wire = wire_columns(scheme, b)
        self.decoded, self.undecodable = decode_columns(self.wire)
        self._want = {}

    def want(self, key_fmt="affine", sig_fmt=None):
        """The reference statuses with the keys taken from `key_fmt` and the signatures from `sig_fmt` (default: the same):
        the C oracle on the affine points (ext is the same points) or on what the wire strings decode to, 3 where one does
        not decode."""
        sig_fmt = sig_fmt or key_fmt
        tag = (key_fmt == "wire", sig_fmt == "wire")
        if tag not in self._want:
            wire_cols = (KEYCOLS[self.scheme] if tag[0] else []) + (RCOLS[self.scheme] if tag[1] else [])
            b = {k: (self.decoded[k] if k in wire_cols else v) for k, v in self.affine.items()}
            st = oracle_verify(self.scheme, b).copy()
            for k in wire_cols:
                st[self.undecodable[k]] = 3
            st.setflags(write=False)
            self._want[tag] = st
        return self._want[tag]

    def key_arrays(self, fmt):
        """the key columns as the calls of `fmt` take them: affine / ext one array per column, wire one array"""
        if fmt == "wire":
            return [np.ascontiguousarray(np.concatenate([self.wire[k] for k in KEYCOLS[self.scheme]], 1))]
        return [(self.ext if fmt == "ext" else self.affine)[k] for k in KEYCOLS[self.scheme]]

    def sig_arrays(self, fmt):
        """the signature columns and the messages as KeySet.verify takes them"""
        b = self.affine
        if fmt == "wire":
            return [np.ascontiguousarray(np.concatenate([b["u"]] + [self.wire[k] for k in RCOLS[self.scheme]], 1)), b["m"]]
        return [b["u"]] + [(self.ext if fmt == "ext" else b)[k] for k in RCOLS[self.scheme]] + [b["m"]]

    def arrays(self, fmt):
        """the arguments of Engine.verify / verify_ext / verify_wire"""
        if fmt == "wire":
            return [self.sig_arrays(fmt)[0], self.key_arrays(fmt)[0], self.affine["m"]]
        src = self.ext if fmt == "ext" else self.affine
        return [src.get(k, self.affine[k]) for k in ARG_ORDER[self.scheme]]


@functools.lru_cache(None)
def forms(scheme):
    f = Forms(scheme, battery(scheme)[0])
    for fmt in FORMATS:
        count_classes(scheme, fmt, f)
    return f


def carried(scheme, fmt, f):
    """Per item: the format's own bytes still carry what defines the item.  affine: always.  ext: every point column gives back
    its affine point when U and V are divided by Z (a row with a coordinate >= q: verbatim with Z = 1).  wire: every point
    column decodes back to its affine point, or is undecodable where the affine point has a coordinate >= q; an off-curve point
    has no encoding, so such an item is not carried in wire."""
    held = np.ones(f.n, bool)
    if fmt == "affine":
        return held
    for k in point_cols(scheme):
        big = non_canonical_rows(f.affine[k])
        for i in range(f.n):
            if fmt == "ext":
                U, V, Z = (to_int(f.ext[k][i, j:j + 32]) for j in (0, 32, 64))
                if big[i]:
                    ok = Z == 1 and f.ext[k][i, :64].tobytes() == f.affine[k][i].tobytes()
                else:
                    zi = pow(Z, Q - 2, Q)
                    ok = 0 < Z < Q and U < Q and V < Q and (U * zi % Q, V * zi % Q) == to_pt(f.affine[k][i])
            else:
                ok = bool(f.undecodable[k][i]) if big[i] else (not f.undecodable[k][i] and f.decoded[k][i].tobytes() == f.affine[k][i].tobytes())
            held[i] &= ok
    return held


def count_classes(scheme, fmt, f):
    classes = battery(scheme)[1]
    held = carried(scheme, fmt, f)
    counts = {c: 0 for c in CLASSES}
    for i, c in enumerate(classes):
        counts[c] += int(held[i])
    CLASS_COUNTS[(scheme, fmt)] = counts


def assert_class_counts():
    """Every class is there in every scheme and format; the classes whose points all lie on the curve (grid, coinciding points,
    exact) are carried whole by every format."""
    for scheme in SCHEMES:
        forms(scheme)
        for fmt in FORMATS:
            counts = CLASS_COUNTS[(scheme, fmt)]
            for cls in CLASSES:
                assert counts[cls] > 0, (scheme, fmt, cls)
            for cls in ("torsion_grid", "degenerate", "exact"):
                assert counts[cls] == CLASS_COUNTS[(scheme, "affine")][cls], (scheme, fmt, cls)
        assert sum(CLASS_COUNTS[(scheme, "affine")].values()) == sum(CLASS_COUNTS[(scheme, "ext")].values()) == forms(scheme).n
        assert sum(CLASS_COUNTS[(scheme, "wire")].values()) < forms(scheme).n          # the off-curve items


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def tiled(b, want, reps):
    """The batch `reps` times over (a dict or a list of arrays).  Tiling multiplies every key's multiplicity by `reps` and
    changes no item, so the statuses tile with it."""
    if isinstance(b, dict):
        return {k: np.tile(v, (reps, 1)) for k, v in b.items()}, np.tile(want, reps)
    return [np.tile(v, (reps, 1)) for v in b], np.tile(want, reps)


def reps_for(n_items, at_least):
    """the smallest number of copies that reaches `at_least` items"""
    return -(-at_least // n_items)


def distinct_keys(key_columns):
    """The number of distinct key byte strings per key column (a list of (n, w) arrays): what the key-table decision counts
    (at most n / 128 in every column: wide windows; at most n / 16: narrow ones; more: no tables)."""
    return [len(np.unique(np.ascontiguousarray(c), axis=0)) for c in key_columns]


def wire_key_columns(pk):
    return [pk[:, i:i + 32] for i in range(0, pk.shape[1], 32)]


# ---- batches derived from the battery ----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def narrow_forms(scheme, n_filler=None):
    """The battery beside `n_filler` items of helpers.make_batch under as many keys of their own (signed and spoilt by the C
    oracle: no Python curve arithmetic), so that tiled to the smallest size at which the key tables engage every key column has
    more than n / 128 distinct keys and the engine's own decision is the narrow windows.  The grid's items are reused as they
    are; growing the grid instead would cost its Python-oracle construction several times over."""
    n_filler = n_filler or (640 if scheme == "single" else 320)
    filler = make_batch(scheme, n_filler, seed=0xF111, n_keys=n_filler)
    return Forms(scheme, concat(battery(scheme)[0], filler), seed=0xF1)


@functools.lru_cache(None)
def twin_forms(scheme):
    """The battery with every other distinct key of every key column replaced by its twin on all the items that carry it:
    the same prime-order part with another torsion component -- a clean key gains a component of order 4 (valid -> not), a
    key with torsion loses it (not valid -> valid) -- so the bytes are distinct and the validity flips.  Keys that are off the
    curve, not canonical or of small order (their prime-order part is the identity: no twin is valid) stay.
    -> (Forms, twins made, twins whose validity by the Python oracle's point_is_valid differs from their original's)"""
    b = {k: v.copy() for k, v in battery(scheme)[0].items()}
    e = 8 * pow(8, -1, R)                                       # 1 mod r, 0 mod 8 (NOT reduced mod r): e * P is the prime-order part of P
    assert e % R == 1 and e % 8 == 0 and e < 1 << 256
    t4 = o.mul(torsion_generator(), 2)
    made = flipped = 0
    for name in KEYCOLS[scheme]:
        uniq, inv = np.unique(b[name], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for j in range(0, len(uniq), 2):
            p = to_pt(uniq[j])
            if p[0] >= Q or p[1] >= Q or not o.is_on_curve(p):
                continue
            prime = o.mul(p, e)
            if prime == o.IDENTITY:
                continue
            twin = o.add(p, t4) if prime == p else prime
            assert twin != p and o.is_on_curve(twin)
            b[name][inv == j] = pt_bytes(twin)
            made += 1
            flipped += int(o.point_is_valid(p) != o.point_is_valid(twin))
    return Forms(scheme, b, seed=0xF2), made, flipped


@functools.lru_cache(None)
def valid_only(scheme, n, seed=0x600D):
    """n valid items under n keys of their own (no key of the battery among them)"""
    b = make_batch(scheme, n, seed=seed, n_keys=n, mix=False)
    assert (oracle_verify(scheme, b) == 0).all()
    return b


def registered(scheme, f, fmt="affine"):
    """The distinct keys of a Forms in `fmt` as Engine.keyset takes them and every item's index among them.
    -> ([key arrays], idx, [the first item of every key])"""
    cols = f.key_arrays(fmt)
    cat = np.ascontiguousarray(np.concatenate(cols, 1))
    uniq, first, inv = np.unique(cat, axis=0, return_index=True, return_inverse=True)
    widths = np.cumsum([0] + [c.shape[1] for c in cols])
    keys = [np.ascontiguousarray(uniq[:, widths[i]:widths[i + 1]]) for i in range(len(cols))]
    return keys, inv.reshape(-1).astype(np.uint32), first


def key_status_reference(scheme, f, fmt, first):
    """The oracle's status of every registered key, from the item that carries it first: 3 a coordinate >= q or an encoding that
    does not decode, 1 a point that is not `is_valid` (off the curve, the identity, with torsion), else 0."""
    import jjs_oracle_c as oc
    out = np.zeros(len(first), np.uint8)
    for k in KEYCOLS[scheme]:
        pts = (f.decoded if fmt == "wire" else f.affine)[k][first]
        malformed = f.undecodable[k][first] if fmt == "wire" else non_canonical_rows(pts)
        flags = oc.point_flags(np.where(malformed[:, None], pt_bytes(o.G)[None], pts))
        # jjo_point_flags: bit 0 on the curve, bit 1 torsion-free, bit 2 the identity
        out = np.maximum(out, np.where(malformed, 3, np.where(flags == 3, 0, 1)).astype(np.uint8))
    return out


def check_new_classes_against_python_oracle(scheme):
    """exact and precedence, item by item: the C oracle's status, the Python oracle's and the status the construction
    intends agree."""
    b, classes = battery(scheme)
    want = forms(scheme).want()
    ex, pr = class_rows(scheme, "exact"), class_rows(scheme, "precedence")
    assert len(ex) == len(exact_plans(scheme)) and (want[ex] == 1).all(), (scheme, want[ex])
    assert want[pr].tolist() == precedence_batch(scheme)[2], (scheme, want[pr])
    assert set(want[pr].tolist()) == {1, 3}
    for i in np.concatenate([ex, pr]):
        assert py_verify(scheme, b, int(i)) == want[i], (scheme, classes[i], int(i))

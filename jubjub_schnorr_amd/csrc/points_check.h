// `is_valid` for its own sake (include/jjs_gpu.h jjs_keys_check / jjs_signatures_check): the predicate every
// verification computes on the way -- coordinates in range, on the curve, not the identity, torsion-free -- for keys and
// signatures that arrive from outside and are not to be verified yet, and the canonical affine point of every column as an
// optional output (the bulk `from_bytes` / `to_hash_inputs`).  Reference: PublicKey::is_valid src/keys/public.rs:159-164 and its
// five siblings.
//
// One lane per POINT: an item with two points (a double or var-gen key, a double signature) takes two adjacent lanes.  The lane
// of a point computes that point's status in one of three ways, by the format of the column:
//   affine  range test, then affine_on_curve, affine_is_identity and is_torsion_free, all three run unconditionally and ANDed
//           (the residue test is defined for on-curve points other than the identity only; on anything else its answer is
//           discarded, and it is straight-line arithmetic, so it can be run on anything);
//   ext     the same on (U : V : Z) WITHOUT an inversion: pairing_is_trivial takes projective input (verify_core.h: the affine
//           expression has the denominator Z^48, an 8th power), the curve equation is (V^2 - U^2) Z^2 == Z^4 + d U^2 V^2 and the
//           identity is U == 0 and V == Z.  Z == 0 is no point of the curve: status 1 whatever the other tests say.  A call
//           that wants the affine points runs the shared-inversion normaliser (normalize.h, plain mode) in front instead and
//           this pass in affine mode over its output, with the normaliser's per-item flags as `bad`;
//   wire    decompress_point (one square root), which yields points on the curve by construction, then the identity and the
//           residue test on the decoded coordinates.
// Status of a point: 3 a coordinate (for ext also Z) >= q or an encoding decompress_point refuses; 1 not 3 and not `is_valid`;
// 0 `is_valid`.  Status of an item: the worst of its points (3 > 1 > 0, as ks_key_status), and 3 for a signature's scalar >= r.
// The two lanes of an item are adjacent lanes of one wave, so the kernel combines them with one lane exchange (pc_item_status
// takes both); there is no status byte in memory that two lanes meet at and no second pass.  The lane that ran a point writes
// that point's output row, and zero bytes over it once the item's status is known to be 3.
//
// All of it is JJS_HD: tests/hostbuild/points_check_harness.cpp runs these functions on the CPU.
#pragma once
#include "decode.h"
#include "normalize.h"

namespace jjs {

enum : uint32_t { PC_AFFINE = 0, PC_EXT = 1, PC_WIRE = 2 };

struct points_check_params {
    uint32_t n_pts;       // points, and lanes, per item: 1 or 2
    uint32_t in_place;    // non-zero: out[k] already holds the rows (the normaliser wrote them); only those of a status-3 item are rewritten
    fe_src src[2];        // point k of item i: affine u at off, v at off + 32; ext U, V, Z at off, + 32, + 64; wire 32 bytes at off
    fe_src scalar;        // a signature's u (base null: the items are keys)
    const uint8_t* bad;   // nullable, n bytes: non-zero when the normaliser in front found a coordinate of item i >= q
    uint8_t* out[2];      // nullable, n x 64: the canonical affine point of column k
    uint8_t* u_out;       // nullable, n x 32: the scalar copied
    uint8_t* status;      // nullable, n bytes
    unsigned long long* tally;   // nullable, 4 counters
    uint64_t n;
    dlog_tables dlog;     // wire
};

// One call's columns as the kernel takes them -- the point columns of an item, a signature's scalar, the outputs -- from the
// columns of the entry points (include/jjs_gpu.h); format: PC_*, which count as JJS_FORMAT_*.
struct points_check_call {
    uint32_t format, n_pts;
    fe_src src[2], scalar;
    uint8_t *out[2], *u_out;
};
// keys of `cols` points: affine / ext K0, K1 (n x 64 / n x 96 each), wire K0 alone (n x 32 cols)
inline points_check_call pc_keys_call(uint32_t cols, uint32_t format, const void* K0, const void* K1, void* A0_out, void* A1_out) {
    points_check_call Q{};
    Q.format = format; Q.n_pts = cols;
    if (format == PC_WIRE) {
        for (uint32_t k = 0; k < cols; ++k) Q.src[k] = fe_src{(const uint8_t*)K0, 32 * cols, 32 * k};
    } else {
        const uint32_t w = format == PC_EXT ? 96u : 64u;
        Q.src[0] = fe_src{(const uint8_t*)K0, w, 0};
        Q.src[1] = fe_src{(const uint8_t*)K1, w, 0};
    }
    Q.out[0] = (uint8_t*)A0_out; Q.out[1] = (uint8_t*)A1_out;
    return Q;
}
// signatures of n_r R points: affine / ext s0 = u, s1 = R, s2 = R'; wire s0 alone (u || R (|| R'))
inline points_check_call pc_signatures_call(uint32_t n_r, uint32_t format, const void* s0, const void* s1, const void* s2, void* u_out, void* R_out,
                                            void* Rp_out) {
    points_check_call Q{};
    Q.format = format; Q.n_pts = n_r;
    if (format == PC_WIRE) {
        const uint32_t stride = 32 + 32 * n_r;
        Q.scalar = fe_src{(const uint8_t*)s0, stride, 0};
        for (uint32_t k = 0; k < n_r; ++k) Q.src[k] = fe_src{(const uint8_t*)s0, stride, 32 + 32 * k};
    } else {
        const uint32_t w = format == PC_EXT ? 96u : 64u;
        Q.scalar = fe_src{(const uint8_t*)s0, 32, 0};
        Q.src[0] = fe_src{(const uint8_t*)s1, w, 0};
        Q.src[1] = fe_src{(const uint8_t*)s2, w, 0};
    }
    Q.u_out = (uint8_t*)u_out; Q.out[0] = (uint8_t*)R_out; Q.out[1] = (uint8_t*)Rp_out;
    return Q;
}
inline points_check_params pc_params(const points_check_call& Q, uint64_t n, uint8_t* status, unsigned long long* tally, const dlog_tables& T) {
    points_check_params C{};
    C.n_pts = Q.n_pts; C.scalar = Q.scalar; C.u_out = Q.u_out;
    C.status = status; C.tally = tally; C.n = n; C.dlog = T;
    for (uint32_t k = 0; k < Q.n_pts; ++k) { C.src[k] = Q.src[k]; C.out[k] = Q.out[k]; }
    return C;
}
// extended points whose affine form is wanted: the normaliser runs in front and the pass in affine mode over its output
inline bool pc_normalises(const points_check_call& Q) { return Q.format == PC_EXT && (Q.out[0] || Q.out[1]); }
inline void pc_over_normalised(points_check_params& C, const normalize_params& N) {
    for (uint32_t k = 0; k < C.n_pts; ++k) C.src[k] = fe_src{N.out[k], 64, 0};
    C.bad = N.bad; C.in_place = 1;
}

JJS_HD uint32_t pc_status(bool malformed, bool valid) { return malformed ? (uint32_t)ST_MALFORMED : (valid ? (uint32_t)ST_OK : (uint32_t)ST_INVALID_POINT); }

JJS_HD uint32_t pc_affine_point(const words8& uw, const words8& vw) {
    const bool canonical = words_lt(uw, JJS_Q_WORDS) && words_lt(vw, JJS_Q_WORDS);
    const fe_n u = fq_from_words(uw), v = fq_from_words(vw);
    const bool on = affine_on_curve(u, v), id = affine_is_identity(u, v), tf = is_torsion_free(u, v);
    return pc_status(!canonical, on & !id & tf);
}

// (V^2 - U^2) Z^2 == Z^4 + d U^2 V^2: the affine equation v^2 - u^2 = 1 + d u^2 v^2 times Z^4
JJS_HD bool ext_on_curve(const fe_n& U, const fe_n& V, const fe_n& Z) {
    const fe_n u2 = fq_sqr(U), v2 = fq_sqr(V), z2 = fq_sqr(Z);
    const fe_n lhs = fq_mul(fq_sub(v2, u2), z2);
    auto rhs = fq_norm(fq_add(fq_mul(fq_mul(u2, v2), fe_from_const<1, 1>(JJS_D)), fq_sqr(z2)));     // <1,4>
    return fq_eq(rhs, lhs);
}
JJS_HD uint32_t pc_ext_point(const words8& Uw, const words8& Vw, const words8& Zw) {
    const bool canonical = words_lt(Uw, JJS_Q_WORDS) && words_lt(Vw, JJS_Q_WORDS) && words_lt(Zw, JJS_Q_WORDS);
    const bool z_zero = words_are_zero(Zw);
    const fe_n U = fq_from_words(Uw), V = fq_from_words(Vw), Z = fq_from_words(Zw);
    const bool on = ext_on_curve(U, V, Z), id = fq_is_zero(U) && fq_eq(V, Z), tf = pairing_is_trivial(U, V, Z);
    return pc_status(!canonical, z_zero ? false : (on & !id & tf));
}

// d: what decompress_point decoded (the identity for an encoding it refuses, which gets status 3)
JJS_HD uint32_t pc_wire_point(const decoded_point& d) {
    const fe_n fu = fq_from_words(d.u), fv = fq_from_words(d.v);
    const bool id = affine_is_identity(fu, fv), tf = is_torsion_free(fu, fv);
    return pc_status(!d.ok, !id & tf);
}

JJS_HD void pc_store_row(uint8_t* out, uint64_t item, bool zero, const words8& u, const words8& v) {
    words8 a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) { a.w[i] = zero ? 0u : u.w[i]; b.w[i] = zero ? 0u : v.w[i]; }
    store_words(out, 2 * item, a);
    store_words(out, 2 * item + 1, b);
}
// The lane of point k of `item`: the point's status, with the item-wide findings this lane is the one to look at folded in (the
// normaliser's flag; on lane 0 the scalar).  Where the mode has the point's affine coordinates (affine, wire) and the caller
// wants them, the lane writes its row as soon as it has it -- zero bytes when the point itself is malformed -- so that the
// sixteen words need not live through the residue test; pc_finish_lane zeroes it again should the item turn out malformed.
// `write`: off for a lane beyond the end of the call, which redoes the last point.
// The column is chosen field by field: indexing the kernel-argument struct with a run-time index would make the compiler copy
// it to scratch memory.
template <uint32_t MODE>
JJS_HD uint32_t pc_point_lane(const points_check_params& C, uint64_t item, uint32_t k, bool write) {
    fe_src s = C.src[0];
    if (k) { s.base = C.src[1].base; s.stride = C.src[1].stride; s.off = C.src[1].off; }
    uint8_t* out = k ? C.out[1] : C.out[0];
    const bool row = write && out && !C.in_place;
    uint32_t st;
    if (MODE == PC_WIRE) {
        const decoded_point d = decompress_point(load_words(s, item), C.dlog);
        if (row) pc_store_row(out, item, !d.ok, d.u, d.v);
        st = pc_wire_point(d);
    } else if (MODE == PC_EXT) {
        st = pc_ext_point(load_words(s, item), load_words(s, item, 32), load_words(s, item, 64));
    } else {
        const words8 u = load_words(s, item), v = load_words(s, item, 32);
        st = pc_affine_point(u, v);
        if (row) pc_store_row(out, item, st == ST_MALFORMED, u, v);
    }
    if (C.bad && C.bad[item]) st = ST_MALFORMED;
    if (k == 0 && C.scalar.base && !words_lt(load_words(C.scalar, item), JJS_FR_WORDS)) st = ST_MALFORMED;
    return st;
}
JJS_HD uint32_t pc_item_status(uint32_t a, uint32_t b) { return a > b ? a : b; }

// What the lane of point k writes once the item's status is known: zero bytes over its row when the item is malformed (its own
// point need not be: the other point, the scalar, the normaliser's flag), and on lane 0 the scalar or zero bytes.
JJS_HD void pc_finish_lane(const points_check_params& C, uint64_t item, uint32_t k, uint32_t item_status) {
    const bool zero = item_status == ST_MALFORMED;
    words8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z.w[i] = 0u;
    uint8_t* out = k ? C.out[1] : C.out[0];
    if (out && zero) {
        store_words(out, 2 * item, z);
        store_words(out, 2 * item + 1, z);
    }
    if (k == 0 && C.u_out) store_words(C.u_out, item, zero ? z : load_words(C.scalar, item));
}

}  // namespace jjs

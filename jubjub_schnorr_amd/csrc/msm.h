// Bucket multi-scalar multiplication (Pippenger) for the batch verdict (batch_verdict.h, include/jjs_gpu.h jjs_verify_all_*).
//
//   sum_t s_t * (+-P_t)    over terms t: affine points as cached addends, scalars below 2^252
//
// Signed windows of c bits (c <= MSM_MAX_WINDOW): W = ceil(253 / c) windows, digits in [-2^(c-1), 2^(c-1)) and an unsigned
// top digit in [0, 2^(c-1)] (s < 2^252 and cW >= 253 keep it there), so window j has B = 2^(c-1) buckets, bucket k holding
// the terms whose digit j is +-(k + 1).  The steps, each a function here that the device runs one lane per unit and the CPU
// build runs in a loop:
//   digits     msm_digit_step: digit j of a term from digit j-1's carry (zero digits go to no bucket);
//   sort       a counting sort of (window, |digit|) -> the term with its sign (bit 31): count, exclusive scan, scatter;
//   buckets    msm_bucket: one lane per bucket adds its terms with mixed additions (ext + affine cached addend, 7 products);
//   segments   msm_segment: window j's buckets cut into K segments of L = B / K; a segment's lane takes the running sum
//              from its top bucket down, sum_{k in seg} (k + 1) S_k = sum_k (k - lo + 1) S_k + lo * (sum_k S_k) (in the top
//              window slot k weighs (k >> s) + 1: msm_top_split);
//   windows    the segments of a window added (msm_add_ext), then the windows by Horner's rule (c doublings each).
#pragma once
#include "verify_core.h"

namespace jjs {

constexpr int MSM_MAX_WINDOW = 16;
constexpr int MSM_TERM_WORDS = 28;          // Y+X, Y-X, 2dXY of the affine point (9 limbs each), padded to 7 x 16 B
constexpr int MSM_EXT_WORDS = 36;           // an extended point: X, Y, Z, T
constexpr uint32_t MSM_NEG = 0x80000000u;   // sign bit of a sorted entry

JJS_HD int msm_windows(int c) { return (253 + c - 1) / c; }
JJS_HD uint32_t msm_buckets(int c) { return 1u << (c - 1); }
// The top window's digits lie in [0, 2^(252 - c(W-1))]: only 2^(c-1-s) of its B buckets, s = cW - 253.  Each of them is split
// in 2^s slots by the low bits of the term index, so that the top window's terms spread over all B slots as the other
// windows' do (a lane per bucket would otherwise take 2^s times the terms of a lane of another window).
JJS_HD int msm_top_split(int c) { return c * msm_windows(c) - 253; }
// slot of the non-zero digit d of term t in window j, the top window's digits split in 2^s slots each
JJS_HD uint32_t msm_slot_split(int j, int32_t d, uint64_t t, int W, int s) {
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d) - 1u;
    if (j < W - 1) return mag;
    return (mag << s) | (uint32_t)(t & ((1u << s) - 1u));
}
JJS_HD uint32_t msm_slot(int j, int32_t d, uint64_t t, int c, int W) { return msm_slot_split(j, d, t, W, msm_top_split(c)); }
// Bits of the batch verdict's weights for window width c: c * ceil(129 / c) - 1 >= 128, so that a weight's top window is
// as full as the others (a weight of exactly 128 bits would carry 0 or 1 into one more window: half of those terms in
// ONE bucket).
JJS_HD int msm_weight_bits(int c) { return c * ((129 + c - 1) / c) - 1; }

// Scalars that are all weights of msm_weight_bits(c) bits (the R terms of keyset_verdict.h) need only the windows the
// weights reach: ceil(129 / c) of them, the top digit unsigned in [0, 2^(c-1)] like the others' magnitudes (the weight has
// c * W - 1 bits), so the top window is as full as the rest and takes no split.
JJS_HD int msm_short_windows(int c) { return (129 + c - 1) / c; }
// ... their window width for N terms: about eight terms per bucket; every width from 8 to MSM_MAX_WINDOW serves
JJS_HD int msm_pick_short_window(uint64_t N) {
    int lg = 0;
    while (lg < 40 && (1ull << (lg + 1)) <= N) ++lg;
    const int want = lg - 2;
    return want > 16 ? 16 : (want < 8 ? 8 : want);
}
// ... and their segments per window: 64 slots each
JJS_HD uint32_t msm_short_segments(int c) { return msm_buckets(c) > 64u ? msm_buckets(c) / 64u : 1u; }

// c bits of s at bit position pos (pos < 256)
JJS_HD uint32_t msm_bits(const words8& s, int pos, int c) {
    const int wi = pos >> 5, sh = pos & 31;
    const uint64_t lo = word_at(s, wi), hi = wi + 1 < 8 ? word_at(s, wi + 1) : 0u;
    return (uint32_t)(((hi << 32) | lo) >> sh) & ((1u << c) - 1u);
}
// signed digit j of s, given the carry out of digit j-1 (0 for j = 0); updates the carry
JJS_HD int32_t msm_digit_step(const words8& s, int j, int c, int W, uint32_t& carry) {
    const uint32_t b = msm_bits(s, c * j, c) + carry;
    const bool wrap = j < W - 1 && b >= (1u << (c - 1));
    carry = wrap ? 1u : 0u;
    return wrap ? (int32_t)b - (int32_t)(1u << c) : (int32_t)b;
}

// term storage: the cached addend of an affine point
JJS_HD void msm_store_term(uint32_t* dst, const fe_n& u, const fe_n& v) {
    const niels_pt n = to_niels(ext_from_affine(u, v));
    uint32_t w[MSM_TERM_WORDS];
#pragma unroll
    for (int i = 0; i < 9; ++i) { w[i] = n.ypx.l[i]; w[9 + i] = n.ymx.l[i]; w[18 + i] = n.t2d.l[i]; }
    w[27] = 0;
    u32x4* p = reinterpret_cast<u32x4*>(dst);
#pragma unroll
    for (int i = 0; i < MSM_TERM_WORDS / 4; ++i) p[i] = u32x4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
}
// acc + (neg ? -P : P) for the stored affine term P: 7 products (T of the result valid)
JJS_HD ext_pt msm_add_term(const ext_pt& p, const uint32_t* src, bool neg) {
    uint32_t w[MSM_TERM_WORDS];
    const u32x4* q = reinterpret_cast<const u32x4*>(src);
#pragma unroll
    for (int i = 0; i < MSM_TERM_WORDS / 4; ++i) { u32x4 v = q[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
    fe_t ypx, ymx, t2d;
#pragma unroll
    for (int i = 0; i < 9; ++i) { ypx.l[i] = w[i]; ymx.l[i] = w[9 + i]; t2d.l[i] = w[18 + i]; }
    const fe_t n_ymx = fq_select(neg, ypx, ymx), n_ypx = fq_select(neg, ymx, ypx);
    const auto n_t2d = fq_select(neg, fq_neg(t2d), fq_as<2, 6>(t2d));    // -P = (-u, v): the sums swap, 2duv changes sign
    fe_n a = fq_mul_hot(fq_sub(p.y, p.x), n_ymx);
    fe_n b = fq_mul_hot(fq_add(p.y, p.x), n_ypx);
    fe_n c = fq_mul_hot(p.t, n_t2d);
    auto d = fq_dbl(p.z);
    auto e = fq_sub(b, a);
    auto f = fq_norm(fq_sub(d, c));
    auto g = fq_add(d, c);
    auto h = fq_norm(fq_add(b, a));
    ext_pt r;
    r.x = fq_mul_hot(e, f);
    r.z = fq_mul_hot(f, g);
    r.y = fq_mul_hot(g, h);
    r.t = fq_mul_hot(h, e);
    return r;
}
JJS_HD ext_pt msm_add_ext(const ext_pt& a, const ext_pt& b) { return ext_add_niels(a, to_niels(b), false, true); }

JJS_HD void msm_store_ext(uint32_t* dst, const ext_pt& p) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { dst[i] = p.x.l[i]; dst[9 + i] = p.y.l[i]; dst[18 + i] = p.z.l[i]; dst[27 + i] = p.t.l[i]; }
}
JJS_HD ext_pt msm_load_ext(const uint32_t* src) {
    ext_pt p;
#pragma unroll
    for (int i = 0; i < 9; ++i) { p.x.l[i] = src[i]; p.y.l[i] = src[9 + i]; p.z.l[i] = src[18 + i]; p.t.l[i] = src[27 + i]; }
    return p;
}

// bucket `id` (= window * B + k): the sum of its sorted entries [off[id], off[id + 1])
JJS_HD ext_pt msm_bucket(const uint32_t* off, const uint32_t* order, const uint32_t* terms, uint32_t id) {
    ext_pt acc = ext_identity();
    for (uint32_t e = off[id]; e < off[id + 1]; ++e) {
        const uint32_t t = order[e];
        acc = msm_add_term(acc, terms + (size_t)(t & ~MSM_NEG) * MSM_TERM_WORDS, (t & MSM_NEG) != 0);
    }
    return acc;
}
// k * P for a small public k (k < 2^16), double-and-add from the top bit
JJS_HD ext_pt msm_small_mul(const ext_pt& p, uint32_t k) {
    ext_pt acc = ext_identity();
    const niels_pt n = to_niels(p);
    for (int i = 15; i >= 0; --i) {
        acc = ext_double(acc, true);
        if ((k >> i) & 1u) acc = ext_add_niels(acc, n, false, true);
    }
    return acc;
}
// segment `seg` of window j: slots [seg * L, seg * L + L) with weights (k >> s) + 1 (buckets: B extended points per
// window; s = 0 except in the top window, and L a multiple of 2^s)
JJS_HD ext_pt msm_segment(const uint32_t* buckets, uint32_t B, uint32_t j, uint32_t seg, uint32_t L, int s) {
    const uint32_t lo = seg * L;
    ext_pt run = ext_identity(), acc = ext_identity();
    for (uint32_t k = lo + L; k-- > lo;) {
        run = msm_add_ext(run, msm_load_ext(buckets + ((size_t)j * B + k) * MSM_EXT_WORDS));
        if ((k & ((1u << s) - 1u)) == 0) acc = msm_add_ext(acc, run);
    }
    return lo ? msm_add_ext(acc, msm_small_mul(run, lo >> s)) : acc;
}
// sum_j 2^(c j) win[j], Horner's rule from the top window
JJS_HD ext_pt msm_combine(const uint32_t* win, int W, int c) {
    ext_pt acc = ext_identity();
    for (int j = W - 1; j >= 0; --j) {
        for (int i = 0; i < c; ++i) acc = ext_double(acc, true);
        acc = msm_add_ext(acc, msm_load_ext(win + (size_t)j * MSM_EXT_WORDS));
    }
    return acc;
}
// The window width for N terms: about eight terms per bucket, among the widths whose top window needs at most 8 slots per
// digit (cW - 253 <= 3: c = 8, 11, 15, 16; the other widths up to 16 leave the top window 2^7 .. 2^13 times emptier than
// the rest, and a lane per slot would not even that out within a segment of 64 slots).
JJS_HD int msm_pick_window(uint64_t N) {
    int lg = 0;
    while (lg < 40 && (1ull << (lg + 1)) <= N) ++lg;
    const int want = lg - 2;
    return want >= 16 ? 16 : (want >= 15 ? 15 : (want >= 11 ? 11 : 8));
}
// segments per window: L = B / K slots each, 64 or 2^s (the top window's slots per digit) if more, at most B
JJS_HD uint32_t msm_segments(int c) {
    const uint32_t B = msm_buckets(c), split = 1u << msm_top_split(c);
    const uint32_t L = split > 64u ? split : 64u;
    return B > L ? B / L : 1u;
}

// The shape of an MSM with c-bit windows: W windows (the top one's digits split in 2^top_split slots each) of B buckets, cut
// into K segments of L.  msm_shape_full: scalars below 2^252; msm_shape_short: scalars that are all weights of
// msm_weight_bits(c) bits.
struct msm_shape {
    int c, W, top_split;
    uint32_t B, K, L;
};
JJS_HD msm_shape msm_shape_full(int c) { return {c, msm_windows(c), msm_top_split(c), msm_buckets(c), msm_segments(c), msm_buckets(c) / msm_segments(c)}; }
JJS_HD msm_shape msm_shape_short(int c) { return {c, msm_short_windows(c), 0, msm_buckets(c), msm_short_segments(c), msm_buckets(c) / msm_short_segments(c)}; }

}  // namespace jjs

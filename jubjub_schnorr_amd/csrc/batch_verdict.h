// Randomized batch verification (include/jjs_gpu.h jjs_verify_all_*): one verdict for a whole batch.
//
// For item i with weights z_i (and z'_i for the second equation of the double scheme), uniform in [0, 2^k) with
// 128 <= k <= 143 (msm_weight_bits: the window width of the MSM decides k) and drawn from
// ChaCha20 (RFC 8439) keyed with a fresh 32-byte seed per call, the batch is accepted when
//     sum_i z_i (u_i G + c_i PK_i - R_i) [+ sum_i z'_i (u_i G' + c_i PK'_i - R'_i)] == O
// and no item failed a per-item check.  The per-item pass (bv_item, one lane per item) runs prepare_item with every point
// given its own residue test (pairing_is_trivial) and no equation: encodings (u < r, coordinates and m < q), on-curve,
// not-identity, torsion-free, and the challenge c.  It writes the MSM terms of the item -- z_i on -R_i, z_i c_i mod r on PK_i,
// and for the per-item generator z_i u_i mod r on Gen_i -- and returns z_i u_i mod r for the fixed-base part, which is summed
// over the batch and multiplied with the comb table of G (G').  msm.h adds the terms.
//
// Soundness: with every point of order r (the per-item tests), D_i = u_i G + c_i PK_i - R_i lies in the group of prime order
// r ~ 2^252.  If some D_j != O, then for any fixed values of the other weights at most one value of z_j mod r makes the sum
// O (z_j < 2^k < r: distinct weights are distinct mod r), so a batch with a bad item is accepted with probability at most
// 2^-k <= 2^-128.  Torsion is not batched (a random combination
// of elements of the cyclic 2-Sylow subgroup of order 8 cancels with probability up to 1/2), and the equation is not
// cofactored: either would accept what the reference rejects.
#pragma once
#include "msm.h"

namespace jjs {

// ---- ChaCha20 block function (RFC 8439 2.3) ------------------------------------------------------------------------------
JJS_HD uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
#define JJS_QR(a, b, c, d)                          \
    a += b; d ^= a; d = rotl32(d, 16);              \
    c += d; b ^= c; b = rotl32(b, 12);              \
    a += b; d ^= a; d = rotl32(d, 8);               \
    c += d; b ^= c; b = rotl32(b, 7);
JJS_HD void chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                      key[4], key[5], key[6], key[7], counter, nonce[0], nonce[1], nonce[2]};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll 1
    for (int r = 0; r < 10; ++r) {
        JJS_QR(x[0], x[4], x[8], x[12]) JJS_QR(x[1], x[5], x[9], x[13]) JJS_QR(x[2], x[6], x[10], x[14]) JJS_QR(x[3], x[7], x[11], x[15])
        JJS_QR(x[0], x[5], x[10], x[15]) JJS_QR(x[1], x[6], x[11], x[12]) JJS_QR(x[2], x[7], x[8], x[13]) JJS_QR(x[3], x[4], x[9], x[14])
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}
#undef JJS_QR

// the weights of item i, `bits` bits each (128 <= bits <= 160: msm_weight_bits): block i of the keystream (counter = low
// 32 bits of i, nonce word 0 = high bits); z = words 0-4, z' = words 5-9, cut to `bits`
JJS_HD void bv_weights(const uint32_t seed[8], uint64_t item, int bits, words8& z, words8& zp) {
    const uint32_t nonce[3] = {(uint32_t)(item >> 32), 0u, 0u};
    uint32_t b[16];
    chacha20_block(seed, (uint32_t)item, nonce, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t mask = 32 * k + 32 <= bits ? 0xffffffffu : (32 * k >= bits ? 0u : (1u << (bits - 32 * k)) - 1u);
        z.w[k] = k < 5 ? b[k] & mask : 0u;
        zp.w[k] = k < 5 ? b[5 + k] & mask : 0u;
    }
}

// ---- the per-item pass ----------------------------------------------------------------------------------------------------
// Terms of item i: kind k has term index k * n + i.  Kinds: for each equation e, R_e (negated) then PK_e; then Gen for the
// per-item generator.
struct bv_params {
    verify_params V;             // the scheme's descriptor (schemes.h params_*): hash inputs, points, equations, u
    uint32_t seed[8];
    int z_bits;                  // bits of the weights (msm_weight_bits of the MSM's window width)
    uint32_t n_kinds;            // 2 single, 4 double, 3 per-item generator
    uint32_t* terms;             // n_kinds * n cached addends (MSM_TERM_WORDS each)
    uint8_t* scalars;            // n_kinds * n scalars, 32 bytes each
    uint32_t* fail;              // non-zero: some item failed a per-item check (device word)
    uint8_t* partial;            // per block of the pass: sum z u, sum z' u mod r (64 bytes)
};
JJS_HD uint32_t bv_kinds(const verify_params& V) { return V.eq[0].comb ? 2u * V.n_eq : 3u; }
JJS_HD bool bv_kind_negated(const verify_params& V, uint32_t k) { return k < 2u * V.n_eq && (k & 1u) == 0u; }

// One item: the checks, the terms, and z u (z' u) mod r for the fixed generator(s) (zero for the per-item generator, whose
// u goes into a term).  Returns false when the item fails a check; its weights are then zero.
JJS_HD bool bv_item(const bv_params& B, uint64_t item, words8 zu[2]) {
    verify_params P = B.V;
    const uint64_t n = P.n;
    P.n_eq = 0;                                         // no Euclid, no combined test: ...
    P.own_test_mask = (1u << P.n_points) - 1u;          // ... every point its own residue test
    P.c_out = nullptr; P.key_flag = nullptr; P.small_mode = 0;
    const prep_record r = prepare_item(P, item, false);
    const bool ok = !r.malformed && r.valid;
    words8 z[2];
    bv_weights(B.seed, item, B.z_bits, z[0], z[1]);
    const words8 u = load_words(B.V.u, item);
    const bool fixed = B.V.eq[0].comb != nullptr;
    zu[1] = words_zero();
    for (uint32_t e = 0; e < B.V.n_eq; ++e) {
        const words8 w = select_words(ok, z[e], words_zero());
        const eq_desc& E = B.V.eq[e];
        msm_store_term(B.terms + ((2 * e) * n + item) * MSM_TERM_WORDS, load_fq(E.r, item), load_fq(E.r, item, 32));
        store_words(B.scalars, (2 * e) * n + item, w);
        msm_store_term(B.terms + ((2 * e + 1) * n + item) * MSM_TERM_WORDS, load_fq(E.pk, item), load_fq(E.pk, item, 32));
        store_words(B.scalars, (2 * e + 1) * n + item, fr_mul(w, r.c));
        const words8 wu = ok ? fr_mul(w, u) : words_zero();
        zu[e] = fixed ? wu : words_zero();
        if (!fixed) {
            msm_store_term(B.terms + (2 * n + item) * MSM_TERM_WORDS, load_fq(E.gen, item), load_fq(E.gen, item, 32));
            store_words(B.scalars, 2 * n + item, wu);
        }
    }
    return ok;
}

// The verdict from the MSM total and the fixed-base sums: total + (sum z u) G [+ (sum z' u) G'] == O and no failed item.
JJS_HD bool bv_verdict(const verify_params& V, ext_pt total, const words8 zu[2], bool any_failed) {
    for (uint32_t e = 0; e < V.n_eq; ++e)
        if (V.eq[e].comb) total = add_comb_range(total, V.eq[e].comb, zu[e], 0, COMB_WINDOWS, true);
    return ext_is_identity(total) && !any_failed;
}

}  // namespace jjs

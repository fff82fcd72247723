// The signer's half of the multisignature scheme (include/jjs_gpu.h jjs_multisig_round1_dev, jjs_multisig_sign*):
//   sign_round_1   reference src/multisig.rs:169-184   R = r * G, S = s * G, given the two RNG draws
//   sign_round_2   src/multisig.rs:213-257             z = r + s * a - (c * d_i) * sk, behind the structural checks :218-246
// over many transcripts at once, laid out as the combine call takes them.  Like sign_core.h this GENERATES test and benchmark
// material and is NOT constant time: table look-ups and branches depend on the secrets.  Never use it with production keys.
// A signing call runs the front of the combine call on the caller's transcripts and two passes of its own:
//   0     msig_map_item                                                  lane per transcript    (unchanged)
//   k     ms_check_item: encodings, duplicated nonces, repeated keys     lane per participant row, behind pass 0
//   1-3   msig_delin_item, msig_agg_item, msig_commit_item               (unchanged)
//   4     ms_final_item: RSa and c; no column of shares to sum           lane (or eight) per transcript
//   s     ms_share_item: the signer's own checks and the share           lane per signing row
// The check pass sets flags in scratch words that the call clears beforehand.  Several lanes may write one flag, so every
// writer stores the same word with a plain store (as mv_check_item does).  Its scan is quadratic in the transcript's length:
// row i compares itself with the rows behind it (DESIGN.md 6.6 on why that is acceptable).
#pragma once
#include "multisig_core.h"

namespace jjs {

enum : uint32_t { ST_DUPLICATED_NONCE = 7 };

struct msig_sign_params {
    msig_params M;                        // PK, R, S, m, offsets, the scratch of passes 0-4; agg_pk and sig_R are scratch columns here
    uint32_t *bad_enc, *dup_nonce;        // scratch [B]: non-zero: an encoding of the transcript is out of range / two rows share an R or an S
    uint32_t* pk_repeats;                 // scratch [N]: non-zero: the row's key stands at another row of its transcript as well
    const uint32_t* signer_row;           // [n_signing] the global row a signing row belongs to; NULL: signing row j belongs to row j
    const uint8_t *sk, *r, *s;            // n_signing x 32
    uint64_t n_signing;
    uint8_t *z_out, *status;              // n_signing x 32, n_signing bytes
};

JJS_HD bool ms_first16_equal(const uint8_t* col, uint64_t a, uint64_t b) {
    const u32x4 x = *reinterpret_cast<const u32x4*>(col + 64 * a), y = *reinterpret_cast<const u32x4*>(col + 64 * b);
    return x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
}
// rows a and b of an N x 64 column hold the same 64 bytes: the first 16 bytes first, the rest only on a hit
JJS_HD bool ms_same_point(const uint8_t* col, uint64_t a, uint64_t b) {
    if (!ms_first16_equal(col, a, b)) return false;
    const u32x4 *x = reinterpret_cast<const u32x4*>(col + 64 * a), *y = reinterpret_cast<const u32x4*>(col + 64 * b);
    bool same = true;
    for (int k = 1; k < 4; ++k) same = same && x[k].x == y[k].x && x[k].y == y[k].y && x[k].z == y[k].z && x[k].w == y[k].w;
    return same;
}
// the check pass (lane per participant row, behind pass 0)
JJS_HD void ms_check_item(const msig_sign_params& S, uint64_t i) {
    const msig_params& P = S.M;
    const uint32_t t = P.tr_of[i], lo = P.offsets[t], hi = P.offsets[t + 1];
    const fe_src pk{P.PK, 64, 0}, rs{P.R, 64, 0}, ss{P.S, 64, 0}, ms{P.m, 32, 0};
    bool bad = i == lo && !words_lt(load_words(ms, t), JJS_Q_WORDS);
    for (int e = 0; e < 2; ++e) {
        bad = bad || !words_lt(load_words(pk, i, 32u * e), JJS_Q_WORDS) || !words_lt(load_words(rs, i, 32u * e), JJS_Q_WORDS) ||
              !words_lt(load_words(ss, i, 32u * e), JJS_Q_WORDS);
    }
    if (bad) S.bad_enc[t] = 1u;
    bool dup = false, repeats = false;
    for (uint64_t k = i + 1; k < hi; ++k) {
        dup = dup || ms_same_point(P.R, i, k) || ms_same_point(P.S, i, k);
        if (ms_same_point(P.PK, i, k)) { repeats = true; S.pk_repeats[k] = 1u; }
    }
    if (dup) S.dup_nonce[t] = 1u;
    if (repeats) S.pk_repeats[i] = 1u;
}
// pass 4 of a signing call (lane, or eight, per transcript): RSa = sum E_i into the scratch column M.sig_R, c = H(RSa, pk_agg, m)
JJS_HD void ms_final_item(const msig_params& P, uint32_t t, int coop = -1) {
    store_point(P.sig_R, t, sum_points_affine(P.e_pt, P.offsets[t], P.offsets[t + 1]));
    const fe_src sr{P.sig_R, 64, 0}, aggs{P.agg_pk, 64, 0}, ms{P.m, 32, 0};
    fe_n dg = poseidon_digest(5, [&](int e) {
        return e < 2 ? load_fq(sr, t, 32u * (uint32_t)e) : (e < 4 ? load_fq(aggs, t, 32u * (uint32_t)(e - 2)) : load_fq(ms, t));
    }, coop);
    store_w8(P.c_words + 8 * t, truncate250(dg));
}
// k * G is the affine point (u, v) of canonical words: compared projectively, without an inversion
JJS_HD bool ms_comb_is(const uint32_t* comb_g, const words8& k, const fe_src& col, uint64_t row) {
    const ext_pt p = comb_mul(comb_g, k);
    return fq_eq(p.x, fq_mul(load_fq(col, row), p.z)) && fq_eq(p.y, fq_mul(load_fq(col, row, 32), p.z));
}
// the share pass (lane per signing row): the first rule that matches gives the status (include/jjs_gpu.h jjs_multisig_sign_dev)
JJS_HD void ms_share_item(const msig_sign_params& S, uint64_t j) {
    const msig_params& P = S.M;
    const fe_src sks{S.sk, 32, 0}, rs{S.r, 32, 0}, ss{S.s, 32, 0};
    const uint64_t i = S.signer_row ? (uint64_t)S.signer_row[j] : j;
    uint32_t st = ST_OK;
    words8 z = small_words(0);
    if (i >= P.n_total) {
        st = ST_MALFORMED;                                   // nothing is addressed through i
    } else {
        const uint32_t t = P.tr_of[i];
        const words8 sk = load_words(sks, j), r = load_words(rs, j), s = load_words(ss, j);
        if (!words_lt(sk, JJS_FR_WORDS) || !words_lt(r, JJS_FR_WORDS) || !words_lt(s, JJS_FR_WORDS) || S.bad_enc[t]) {
            st = ST_MALFORMED;
        } else if (S.pk_repeats[i] || !ms_comb_is(P.comb_g, sk, fe_src{P.PK, 64, 0}, i) || !ms_comb_is(P.comb_g, r, fe_src{P.R, 64, 0}, i) ||
                   !ms_comb_is(P.comb_g, s, fe_src{P.S, 64, 0}, i)) {
            st = ST_INVALID_TRANSCRIPT;
        } else if (S.dup_nonce[t]) {
            st = ST_DUPLICATED_NONCE;
        } else {
            const words8 a = load_w8(P.a_words + 8 * t), c = load_w8(P.c_words + 8 * t), d = load_w8(P.d_words + 8 * i);
            z = fr_sub_mul(fr_add(r, fr_mul(s, a)), fr_mul(c, d), sk);
        }
    }
    store_words(S.z_out, j, z);
    S.status[j] = (uint8_t)st;
}

// sign_round_1 given the two draws (lane per row): R = r * G, S = s * G; a scalar >= the group order: both rows zero, bad = 1
JJS_HD void ms_round1_item(const uint8_t* r, const uint8_t* s, const uint32_t* comb_g, uint64_t i, uint8_t* R_out, uint8_t* S_out, uint8_t* bad) {
    const words8 rw = load_words(fe_src{r, 32, 0}, i), sw = load_words(fe_src{s, 32, 0}, i);
    const bool ok = words_lt(rw, JJS_FR_WORDS) && words_lt(sw, JJS_FR_WORDS);
    if (bad) bad[i] = ok ? 0 : 1;
    affine_words zero;
    zero.u = small_words(0); zero.v = small_words(0);
    store_point(R_out, i, ok ? to_affine_words(comb_mul(comb_g, rw)) : zero);
    store_point(S_out, i, ok ? to_affine_words(comb_mul(comb_g, sw)) : zero);
}

}  // namespace jjs

// The multisignature batch of multisig_core.h for committees drawn from a registered key set (include/jjs_gpu.h
// jjs_multisig_combine_keyset[_dev]): ragged transcripts as in the inline call, every share's key named by a 4-byte index into
// a JJS_SCHEME_SINGLE key set (keyset.h).  The set keeps, per key, the canonical affine bytes, the flags and the window tables
// {0 .. 2^(w-1)} * 2^(w i) * PK at w = KEYSET_WINDOW == MG_WINDOW, so the two multiplications by PK_i of the inline call
// (d_i * PK_i in pass 1, (c d_i mod r) * PK_i in pass 5) become walks of 43 additions over stored tables; d_i changes with the
// subset, so nothing else can be stored.  The passes:
//   0   msig_map_item                                                   lane per transcript   (inline body, unchanged)
//   g   mk_gather_item: the key bytes of every row into a PK column in the scratch, the row's table index, and the
//       transcript of an unusable row marked refused                    lane per share
//   1   mk_delin_item: the hash of msig_delin_item on the gathered bytes, D_i = d_i * PK_i over the tables   lane (or eight) per share
//   2-4 msig_agg_item, msig_commit_item, msig_final_item                (inline bodies, msig_params::PK = the gathered column)
//   5   mk_share_item: msig_share_item less the range tests of PK, the product over the tables   lane per share
//   6   msig_verdict_item                                               (inline body)
//   7   mk_refuse_item: a refused transcript gets status 3 on every share, transcript status 3, and agg_pk, sig_u, sig_R zeroed
// The gather runs BEHIND pass 0 and takes a row's transcript from tr_of; it does not search the offsets.
//
// A row is usable when key_idx[i] < n_keys and the key's status is 0 (KT_KEY_VALID without KT_KEY_MALFORMED).  An unusable row
// gets the stand-in key (0, 1) and table index 0 before any key or table is addressed, so no lane reads outside the set; the
// tables of an invalid key are zero-filled, walking them is harmless, and pass 7 discards whatever its transcript computed.
// For a transcript whose rows are all usable the outputs are the inline call's, byte for byte: only the two products by PK_i
// change method, a registered valid key is on the curve, so the walk and the in-lane multiplication give the same group
// element, and every comparison and output is made in affine form.  As in msig_group.h, c * d_i is reduced mod r BEFORE the
// point is multiplied (see the top of that file).
#pragma once
#include "keyset.h"
#include "msig_group.h"

namespace jjs {

static_assert(MG_WINDOW == KEYSET_WINDOW, "the share pass walks the key set's tables with the signer groups' window");

struct msig_keyset_params {
    msig_params M;               // the call; M.PK is the gathered column (pk_col)
    const uint32_t* key_idx;     // [N] the caller's indices
    uint32_t n_keys, pad_;
    const uint8_t* keys;         // the set: n_keys x 64 canonical affine
    const uint8_t* flags;        // n_keys KT_KEY_*
    const uint32_t* tables;      // [n_keys][positions][table words]
    uint8_t* pk_col;             // scratch: N x 64
    uint32_t* row_key;           // scratch: [N] the table index of a row (0 for an unusable row)
    uint32_t* refused;           // scratch: [B] non-zero: the transcript names an unusable row (cleared by the call)
};

JJS_HD bool mk_row_usable(const msig_keyset_params& K, uint32_t idx) {
    return idx < K.n_keys && (K.flags[idx] & (KT_KEY_VALID | KT_KEY_MALFORMED)) == KT_KEY_VALID;
}
// the gather (lane per share, behind pass 0)
JJS_HD void mk_gather_item(const msig_keyset_params& K, uint64_t i) {
    const uint32_t idx = K.key_idx[i];
    const bool usable = mk_row_usable(K, idx);
    const uint32_t row = usable ? idx : 0u;                    // the stand-in row, before anything of the set is addressed
    const fe_src ks{K.keys, 64, 0};
    store_words(K.pk_col, 2 * i, select_words(usable, load_words(ks, row), small_words(0)));
    store_words(K.pk_col, 2 * i + 1, select_words(usable, load_words(ks, row, 32), small_words(1)));
    K.row_key[i] = row;
    if (!usable) K.refused[K.M.tr_of[i]] = 1u;                 // a plain store: every writer stores the same word
}
JJS_HD key_column mk_column(const msig_keyset_params& K) {
    key_column C{};
    C.tables = const_cast<uint32_t*>(K.tables);
    return C;
}
// pass 1: d_i as msig_delin_item hashes it, D_i = d_i * PK_i over the set's tables
JJS_HD void mk_delin_item(const msig_keyset_params& K, uint64_t i, int coop = -1) {
    const msig_params& P = K.M;
    const uint32_t t = P.tr_of[i], lo = P.offsets[t], hi = P.offsets[t + 1];
    const int n_in = 2 + 2 * (int)(hi - lo);
    const fe_src pk{P.PK, 64, 0};
    fe_n dg = poseidon_digest_tagged(n_in, msig_tag(P, t, hi - lo, 0, n_in), [&](int e) {
        return e < 2 ? load_fq(pk, i, 32u * (uint32_t)e) : load_fq(pk, lo + (uint64_t)((e - 2) >> 1), 32u * (uint32_t)(e & 1));
    }, coop);
    const words8 d = truncate250(dg);
    store_w8(P.d_words + 8 * i, d);
    store_ext(P.dpk + EXT_WORDS * i, kt_add_scalar(ext_identity(), mk_column(K), K.row_key[i], d, KEYSET_WINDOW));
}
// pass 5: the equation of msig_share_item over the set's tables; the range tests are its own, less those of PK (registration)
JJS_HD void mk_share_item(const msig_keyset_params& K, uint64_t i) {
    const msig_params& P = K.M;
    const uint32_t t = P.tr_of[i];
    const fe_src zs{P.z, 32, 0}, rs{P.R, 64, 0}, ss{P.S, 64, 0}, ms{P.m, 32, 0};
    const words8 z = load_words(zs, i);
    bool malformed = !words_lt(z, JJS_FR_WORDS) || !words_lt(load_words(ms, t), JJS_Q_WORDS);
    for (int e = 0; e < 2; ++e)
        malformed = malformed || !words_lt(load_words(rs, i, 32u * e), JJS_Q_WORDS) || !words_lt(load_words(ss, i, 32u * e), JJS_Q_WORDS);
    const words8 cd = fr_mul(load_w8(P.c_words + 8 * t), load_w8(P.d_words + 8 * i));
    ext_pt lhs = kt_add_scalar(ext_identity(), mk_column(K), K.row_key[i], cd, KEYSET_WINDOW);   // T valid: the comb additions need it
    lhs = add_comb(lhs, P.comb_g, z);
    const ext_pt e = load_ext(P.e_pt + EXT_WORDS * i);
    const bool ok = fq_eq(fq_mul(lhs.x, e.z), fq_mul(e.x, lhs.z)) && fq_eq(fq_mul(lhs.y, e.z), fq_mul(e.y, lhs.z));
    P.share_status[i] = (uint8_t)(malformed ? (uint32_t)ST_MALFORMED : (ok ? (uint32_t)ST_OK : (uint32_t)ST_INVALID_SHARE));
}
// pass 7 (lane per transcript, behind the verdicts): what a refused transcript gets
JJS_HD void mk_refuse_item(const msig_keyset_params& K, uint32_t t) {
    if (!K.refused[t]) return;
    const msig_params& P = K.M;
    for (uint32_t i = P.offsets[t]; i < P.offsets[t + 1]; ++i) P.share_status[i] = (uint8_t)ST_MALFORMED;
    if (P.transcript_status) P.transcript_status[t] = (uint8_t)ST_MALFORMED;
    store_words(P.sig_u, t, small_words(0));
    for (uint64_t k = 0; k < 2; ++k) {
        store_words(P.agg_pk, 2 * (uint64_t)t + k, small_words(0));
        store_words(P.sig_R, 2 * (uint64_t)t + k, small_words(0));
    }
}

}  // namespace jjs

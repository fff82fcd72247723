// verify_share on its own (include/jjs_gpu.h jjs_multisig_verify_share*, jjs_msig_group_verify_share*,
// jjs_multisig_verify_share_keyset*): the reference's verify_share(share, participant_index, pk_vec, R_vec, S_vec, msg)
// (src/multisig.rs:284-309, 366-387) for Q queries (transcript, slot, z) against B transcripts laid out as the combine call of
// the same route takes them.  The front of that combine call runs unchanged -- inline: msig_kernel passes 0-2; signer group:
// mg_binding_item; key set: the gather, mk_delin_item and pass 2 -- and then, instead of one commitment, one comb and one
// product by PK per ROW:
//   k   msh_check_item: the range tests of the encodings, one flag word per transcript     lane per participant row
//   s   msh_sums_item:  RSa = sum R_i + a * sum S_i, sig_R, c = H(RSa, pk_agg, m)          lane (or eight) per transcript
//   q1  msh_commit_item: E_q = R_j + a * S_j into the query's scratch point               lane per query
//   q2  msh_inline_item / msh_tables_item: z * G + (c * d_j mod r) * PK_j == E_q, the status   lane per query
// s and q1 need a_t alone and write different words, so they share ONE launch (the lanes behind those of the transcripts take
// the queries): the products a * sum S and a * S_j, each a chain of 252 doublings in one lane, then run side by side, and a call
// with few lanes waits for two products in a row, as the combine call does, not three.
// RSa: the combine call sums E_i = R_i + a * S_i over the rows (n products); sum R_i + a * sum S_i is the same group element
// with ONE product.  The complete addition law makes the whole curve a group, and k * P is k-fold addition in it, so
// a * (S_1 + ... + S_n) = a * S_1 + ... + a * S_n for every point of the curve, inside the prime-order subgroup or not -- unlike
// c * (d_j * PK_j), where the two scalars would have to be multiplied mod the order of PK_j (msig_group.h).  sig_R is written in
// affine form, so the two routes give the same bytes.
// The flag words are cleared by the call; several lanes may set one, every writer storing the same word with a plain store.
// A query whose status is 3 or 5 addresses nothing through its indices.
#pragma once
#include "msig_keyset.h"

namespace jjs {

struct msig_share_params {
    msig_params M;                    // the call: PK (inline, key set: the gathered column), R, S, m, offsets, the scratch of the front
                                      // passes, agg_pk (a scratch column; a group's own key, read only), sig_R (the caller's, or a
                                      // scratch column), e_pt = one point per QUERY, comb_g, lane_ws, hash_lanes.  Not used: z,
                                      // share_status, sig_u, transcript_status
    const uint32_t *q_transcript, *q_slot;   // [Q]
    const uint8_t* q_z;               // Q x 32
    uint64_t n_queries;
    uint8_t* q_status;                // Q bytes
    uint32_t* bad;                    // scratch [B]: non-zero: an encoding of the transcript is unusable (for a key-set call the
                                      // gather's `refused` words are these same words)
    uint32_t participants;            // a signer group's n: transcript t owns the rows [t n, (t + 1) n), its aggregate key is row 0
                                      // of M.agg_pk and d_j is d_words[j]; 0: ragged transcripts (M.offsets), key at row t, d_words[row]
    uint32_t check_pk;                // the check pass tests PK as well (inline; registered keys were tested when they were registered)
    const uint32_t* d_words;          // d: [n] of the group, or M.d_words
    const uint32_t* tables;           // the group's or the key set's window tables (msh_tables_item)
    const uint32_t* row_key;          // key set: the table index of a row; NULL: a group, whose table index is the slot
    const uint32_t* tag_a;            // group: [9] the tag of the binding hash
};

// the launch of the sums pass and the first step of the query pass: the lane of query 0 behind `sums_lanes` lanes of transcripts
constexpr uint64_t MSH_QUERY_ALIGN = 64;
JJS_HD constexpr uint64_t msh_first_query_lane(uint64_t sums_lanes) { return (sums_lanes + MSH_QUERY_ALIGN - 1) / MSH_QUERY_ALIGN * MSH_QUERY_ALIGN; }

JJS_HD uint32_t msh_lo(const msig_share_params& X, uint32_t t) { return X.participants ? t * X.participants : X.M.offsets[t]; }
JJS_HD uint32_t msh_hi(const msig_share_params& X, uint32_t t) { return X.participants ? (t + 1) * X.participants : X.M.offsets[t + 1]; }

// the check pass (lane per participant row, behind the map): ms_check_item's range tests without its scan; m is tested where it
// is read, by the transcript's lane and the query's (a transcript without rows has it tested too)
JJS_HD void msh_check_item(const msig_share_params& X, uint64_t i) {
    const msig_params& P = X.M;
    const uint32_t t = X.participants ? (uint32_t)(i / X.participants) : P.tr_of[i];
    const fe_src pk{P.PK, 64, 0}, rs{P.R, 64, 0}, ss{P.S, 64, 0};
    bool bad = false;
    for (int e = 0; e < 2; ++e) {
        bad = bad || !words_lt(load_words(rs, i, 32u * e), JJS_Q_WORDS) || !words_lt(load_words(ss, i, 32u * e), JJS_Q_WORDS);
        if (X.check_pk) bad = bad || !words_lt(load_words(pk, i, 32u * e), JJS_Q_WORDS);
    }
    if (bad) X.bad[t] = 1u;
}
// the sum of rows [lo, hi) of an N x 64 affine column (T valid)
JJS_HD ext_pt msh_sum_column(const uint8_t* col, uint32_t lo, uint32_t hi) {
    const fe_src c{col, 64, 0};
    ext_pt acc = ext_identity();
    for (uint32_t i = lo; i < hi; ++i) acc = ext_add_niels(acc, to_niels(ext_from_affine(load_fq(c, i), load_fq(c, i, 32))), false, true);
    return acc;
}
// the sums pass (lane, or eight, per transcript): RSa = sum R + a * sum S into sig_R, c = H(RSa, pk_agg, m) into c_words.  A flagged
// transcript or one without rows runs the same arithmetic (whatever its bytes are, they only feed field operations) and gets zero rows.
JJS_HD void msh_sums_item(const msig_share_params& X, uint32_t t, uint32_t* ws, int coop = -1) {
    const msig_params& P = X.M;
    const uint32_t lo = msh_lo(X, t), hi = msh_hi(X, t);
    const fe_src sr{P.sig_R, 64, 0}, aggs{P.agg_pk, 64, 0}, ms{P.m, 32, 0};
    const uint64_t agg_row = X.participants ? 0 : t;
    const bool flagged = X.bad[t] != 0u || !words_lt(load_words(ms, t), JJS_Q_WORDS);
    const ext_pt sum_s = msh_sum_column(P.S, lo, hi);
    const fe_n zi = fq_inverse(sum_s.z);
    build_point_table(ws, fq_mul(sum_s.x, zi), fq_mul(sum_s.y, zi));
    const ext_pt as = table_mul(ws, load_w8(P.a_words + 8 * t), true);
    const ext_pt rsa = ext_add_niels(as, to_niels(msh_sum_column(P.R, lo, hi)), false, false);
    const bool nothing = flagged || lo == hi;
    affine_words out = to_affine_words(rsa);
    out.u = select_words(nothing, small_words(0), out.u);
    out.v = select_words(nothing, small_words(0), out.v);
    store_point(P.sig_R, t, out);
    fe_n dg = poseidon_digest(5, [&](int e) {
        return e < 2 ? load_fq(sr, t, 32u * (uint32_t)e) : (e < 4 ? load_fq(aggs, agg_row, 32u * (uint32_t)(e - 2)) : load_fq(ms, t));
    }, coop);
    store_w8(P.c_words + 8 * t, select_words(nothing, small_words(0), truncate250(dg)));
}

// the status a query has before any equation: 3 (rule 1-3), 5 (rule 4), or ST_OK with the row it asks about
JJS_HD uint32_t msh_query_row(const msig_share_params& X, uint64_t q, uint64_t& row) {
    const uint32_t t = X.q_transcript[q], j = X.q_slot[q];
    row = 0;
    if (t >= X.M.n_transcripts || X.bad[t] || !words_lt(load_words(fe_src{X.M.m, 32, 0}, t), JJS_Q_WORDS)) return ST_MALFORMED;
    if (!words_lt(load_words(fe_src{X.q_z, 32, 0}, q), JJS_FR_WORDS)) return ST_MALFORMED;
    const uint32_t lo = msh_lo(X, t), hi = msh_hi(X, t);
    if (j >= hi - lo) return ST_INVALID_TRANSCRIPT;
    row = (uint64_t)lo + j;
    return ST_OK;
}
// query pass, first step: E_q = R_row + a * S_row into the query's point
JJS_HD void msh_commit_item(const msig_share_params& X, uint64_t q, uint32_t* ws) {
    uint64_t row;
    if (msh_query_row(X, q, row) != ST_OK) return;
    msig_commit_share_to(X.M, row, X.q_transcript[q], ws, X.M.e_pt + EXT_WORDS * q);
}
// ... second step, behind it: lhs == E_q, projectively (msig_share_item's comparison), and the status
JJS_HD void msh_finish(const msig_share_params& X, uint64_t q, const ext_pt& lhs) {
    const ext_pt e = load_ext(X.M.e_pt + EXT_WORDS * q);
    const bool ok = fq_eq(fq_mul(lhs.x, e.z), fq_mul(e.x, lhs.z)) && fq_eq(fq_mul(lhs.y, e.z), fq_mul(e.y, lhs.z));
    X.q_status[q] = (uint8_t)(ok ? (uint32_t)ST_OK : (uint32_t)ST_INVALID_SHARE);
}
JJS_HD words8 msh_cd(const msig_share_params& X, uint64_t q, uint64_t row) {
    const uint64_t d_row = X.participants ? (uint64_t)X.q_slot[q] : row;
    return fr_mul(load_w8(X.M.c_words + 8 * (size_t)X.q_transcript[q]), load_w8(X.d_words + 8 * d_row));
}
// inline: the product by PK_row from a table built in the lane
JJS_HD void msh_inline_item(const msig_share_params& X, uint64_t q, uint32_t* ws) {
    uint64_t row;
    const uint32_t st = msh_query_row(X, q, row);
    if (st != ST_OK) { X.q_status[q] = (uint8_t)st; return; }
    const fe_src pk{X.M.PK, 64, 0};
    build_point_table(ws, load_fq(pk, row), load_fq(pk, row, 32));
    ext_pt lhs = table_mul(ws, msh_cd(X, q, row), true);               // T needed by the comb additions
    msh_finish(X, q, add_comb(lhs, X.M.comb_g, load_words(fe_src{X.q_z, 32, 0}, q)));
}
// signer group, key set: one walk over the stored tables (mg_share_item, mk_share_item)
JJS_HD void msh_tables_item(const msig_share_params& X, uint64_t q) {
    uint64_t row;
    const uint32_t st = msh_query_row(X, q, row);
    if (st != ST_OK) { X.q_status[q] = (uint8_t)st; return; }
    key_column C{};
    C.tables = const_cast<uint32_t*>(X.tables);
    const uint32_t key = X.row_key ? X.row_key[row] : X.q_slot[q];
    ext_pt lhs = kt_add_scalar(ext_identity(), C, key, msh_cd(X, q, row), MG_WINDOW);   // T valid: the comb additions need it
    msh_finish(X, q, add_comb(lhs, X.M.comb_g, load_words(fe_src{X.q_z, 32, 0}, q)));
}

}  // namespace jjs

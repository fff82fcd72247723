// Multisig signer groups (include/jjs_gpu.h jjs_msig_group_*): the multisignature batch of multisig_core.h for a committee
// that signs many messages.  Everything the reference derives from the ordered key vector alone (src/multisig.rs:393-429,
// 440-460) is computed ONCE, when the group is registered, and kept on the device:
//   d_i     = H(pk_i, pk_1 .. pk_n) truncated to 250 bits: n hashes of (2 + 2n) / 4 permutations each;
//   agg_pk  = sum d_i * PK_i;
//   tag     the SAFE tag of the binding hash's 3 + 4n inputs (computed for more than JJS_MSIG_MAX_PARTICIPANTS participants);
//   tables  {0 .. 2^(w-1)} * 2^(w i) * PK_i at w = KT_WINDOW_WIDE: the key-table path's tables (key_tables.h), for EVERY key --
//           like the reference, a group does not validate its points.
// A call then takes B transcripts of exactly the group's n participants in the group's order (share (t, j) at row t n + j) and
// runs five passes instead of seven:
//   0  a_t = H(agg_pk, m_t, R, S ...)                         lane (or eight) per transcript   msig_binding_hash
//   1  E = R + a * S                                         lane per share                   msig_commit_share
//   2  RSa = sum E, c = H(RSa, agg_pk, m), u = sum z          lane (or eight) per transcript   msig_final_range
//   3  z * G + (c * d_j mod r) * PK_j == E                     lane per share                   mg_share_item
//   4  the verdict of `combine`                               lane per transcript              msig_verdict_range
// Pass 3 is a comb and ONE walk over the stored tables (43 additions, no doubling, no table built in the lane).
//
// Why the tables are PK_j's and the lane multiplies c by the stored d_j (two Montgomery products mod r, nothing beside 59
// point additions), and not tables of D_j = d_j * PK_j walked with c alone: the reference reduces c * d_j mod r BEFORE it
// multiplies the point (verify_share_with_coefficients, src/multisig.rs:366-387), and c * (d_j * PK_j) is (c d_j) * PK_j
// with the product NOT reduced.  The two agree on the prime-order subgroup only.  Points are not validated, so a key
// PK_j = P + T with T of order 2, 4 or 8 can be registered, and a share under it that the reference accepts (its R or S
// carries the matching small-order part) would be rejected seven times out of eight by the D_j tables.  With PK_j's tables
// and the reduced product the group call computes the inline call's own equation, for every point of the curve.
// (A "key" that is not on the curve at all has no defined outputs on either route: the addition law is a group law only there.)
#pragma once
#include "key_tables.h"
#include "multisig_core.h"

namespace jjs {

constexpr int MG_WINDOW = KT_WINDOW_WIDE;
constexpr size_t MG_TABLE_WORDS_PER_KEY = (size_t)kt_positions(MG_WINDOW) * kt_table_words(MG_WINDOW);
constexpr size_t MG_BASE_WORDS_PER_KEY = (size_t)kt_positions(MG_WINDOW) * KT_BASE_WORDS;

struct msig_group_params {
    msig_params M;                 // the call: z, R, S, m, the outputs, e_pt / a_words / c_words, comb_g, lane_ws, hash_lanes.
                                   // Not used: PK, offsets, tr_of, d_words, dpk, tags, long_tags; agg_pk = the group's (read only)
    uint32_t participants;         // n of the group: transcript t owns the shares [t n, (t + 1) n)
    uint32_t by_participant;       // pass 3: lane k takes share (t, j) = (k % B, k / B) instead of (k / n, k % n), so that a wave
                                   // of 64 lanes walks the tables of one or two keys instead of up to 64
    const uint32_t* d_words;       // [n][8] d_j
    const uint32_t* tables;        // [n][positions][table words]
    const uint32_t* tag_a;         // [9] the tag of the binding hash
};

// what jjs_msig_group_create refuses: no participant, or a coordinate that is not canonical (the per-call range tests of
// msig_share_item then have nothing left to say about PK)
JJS_HD bool mg_keys_acceptable(const uint8_t* PK, uint64_t n) {
    if (!PK || n == 0) return false;
    const fe_src pk{PK, 64, 0};
    bool ok = true;
    for (uint64_t i = 0; i < n; ++i) ok = ok && words_lt(load_words(pk, i), JJS_Q_WORDS) && words_lt(load_words(pk, i, 32), JJS_Q_WORDS);
    return ok;
}
// the same for keys in extended coordinates (n x 96): every key usable -- U, V, Z < q and Z != 0 (normalize.h, poison mode)
JJS_HD bool mg_ext_keys_usable(const uint8_t* PK_ext, uint64_t n) {
    if (!PK_ext || n == 0) return false;
    const fe_src pk{PK_ext, 96, 0};
    bool ok = true;
    for (uint64_t i = 0; i < n; ++i) {
        const words8 z = load_words(pk, i, 64);
        uint32_t any = 0;
        for (int k = 0; k < 8; ++k) any |= z.w[k];
        ok = ok && any != 0 && words_lt(z, JJS_Q_WORDS) && words_lt(load_words(pk, i), JJS_Q_WORDS) && words_lt(load_words(pk, i, 32), JJS_Q_WORDS);
    }
    return ok;
}
// the same for keys in the wire encoding (n x 32): every key decodes (decode.h decompress_point, on the host with tables built
// there); out receives the n x 64 affine keys, which jjs_msig_group_create_wire registers
JJS_HD bool mg_wire_keys_decode(const uint8_t* PK_w, uint64_t n, const dlog_tables& T, uint8_t* out) {
    if (!PK_w || n == 0) return false;
    const fe_src pk{PK_w, 32, 0};
    bool ok = true;
    for (uint64_t i = 0; i < n; ++i) {
        const decoded_point d = decompress_point(load_words(pk, i), T);
        ok = ok && d.ok;
        store_words(out, 2 * i, d.u);
        store_words(out, 2 * i + 1, d.v);
    }
    return ok;
}

// ---- registration ------------------------------------------------------------------------------------------------------------
// (d_j and D_j = d_j * PK_j: msig_delin_item on a one-transcript msig_params; agg_pk: sum_points_affine over the D_j)
// the chain of bases 2^(w i) * PK_j of one key (kt_chain_key without the validity test: a group has none)
JJS_HD void mg_chain_item(const uint8_t* PK, uint32_t j, uint32_t* bases) {
    const fe_src pk{PK, 64, 0};
    ext_pt p = ext_from_affine(load_fq(pk, j), load_fq(pk, j, 32));
    uint32_t* dst = bases + (size_t)j * MG_BASE_WORDS_PER_KEY;
    kt_store_ext(dst, p);
    for (int pos = 1; pos < kt_positions(MG_WINDOW); ++pos) {
#pragma unroll 1
        for (int k = 0; k < MG_WINDOW; ++k) p = ext_double(p, k == MG_WINDOW - 1);
        kt_store_ext(dst + (size_t)pos * KT_BASE_WORDS, p);
    }
}
JJS_HD void mg_table_item(const uint32_t* bases, uint32_t* tables, uint32_t j, uint32_t pos) {
    kt_build_table(tables + (size_t)j * MG_TABLE_WORDS_PER_KEY + (size_t)pos * kt_table_words(MG_WINDOW),
                   kt_load_ext(bases + (size_t)j * MG_BASE_WORDS_PER_KEY + (size_t)pos * KT_BASE_WORDS), kt_entries(MG_WINDOW));
}

// ---- the call ----------------------------------------------------------------------------------------------------------------
JJS_HD fe_n mg_tag(const msig_group_params& G) { return load_tag(G.tag_a, 0); }
JJS_HD void mg_binding_item(const msig_group_params& G, uint32_t t, int coop = -1) {
    const uint64_t n = G.participants;
    msig_binding_hash(G.M, t, t * n, (t + 1) * n, mg_tag(G), G.M.agg_pk, 0, coop);
}
JJS_HD void mg_commit_item(const msig_group_params& G, uint64_t i, uint32_t* ws) { msig_commit_share(G.M, i, (uint32_t)(i / G.participants), ws); }
JJS_HD void mg_final_item(const msig_group_params& G, uint32_t t, int coop = -1) {
    msig_final_range(G.M, t, t * G.participants, (t + 1) * G.participants, G.M.agg_pk, 0, coop);
}
// the share of lane k of pass 3 (see by_participant)
JJS_HD uint64_t mg_share_of_lane(const msig_group_params& G, uint64_t k) {
    if (!G.by_participant) return k;
    const uint64_t B = G.M.n_transcripts;
    return (k % B) * G.participants + k / B;
}
// pass 3: the equation of msig_share_item over the stored tables; the range tests are its own, less those of PK (registration)
JJS_HD void mg_share_item(const msig_group_params& G, uint64_t i) {
    const msig_params& P = G.M;
    const uint32_t t = (uint32_t)(i / G.participants), j = (uint32_t)(i % G.participants);
    const fe_src zs{P.z, 32, 0}, rs{P.R, 64, 0}, ss{P.S, 64, 0}, ms{P.m, 32, 0};
    const words8 z = load_words(zs, i);
    bool malformed = !words_lt(z, JJS_FR_WORDS) || !words_lt(load_words(ms, t), JJS_Q_WORDS);
    for (int e = 0; e < 2; ++e)
        malformed = malformed || !words_lt(load_words(rs, i, 32u * e), JJS_Q_WORDS) || !words_lt(load_words(ss, i, 32u * e), JJS_Q_WORDS);
    const words8 cd = fr_mul(load_w8(P.c_words + 8 * t), load_w8(G.d_words + 8 * (size_t)j));
    key_column C{};
    C.tables = const_cast<uint32_t*>(G.tables);
    ext_pt lhs = kt_add_scalar(ext_identity(), C, j, cd, MG_WINDOW);          // T valid: the comb additions need it
    lhs = add_comb(lhs, P.comb_g, z);
    const ext_pt e = load_ext(P.e_pt + EXT_WORDS * i);
    const bool ok = fq_eq(fq_mul(lhs.x, e.z), fq_mul(e.x, lhs.z)) && fq_eq(fq_mul(lhs.y, e.z), fq_mul(e.y, lhs.z));
    P.share_status[i] = (uint8_t)(malformed ? (uint32_t)ST_MALFORMED : (ok ? (uint32_t)ST_OK : (uint32_t)ST_INVALID_SHARE));
}
JJS_HD void mg_verdict_item(const msig_group_params& G, uint32_t t) {
    msig_verdict_range(G.M, t, t * G.participants, (t + 1) * G.participants);
}

}  // namespace jjs

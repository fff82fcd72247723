// The batch verdict against a registered key set (include/jjs_gpu.h jjs_keyset_verify_all*): batch_verdict.h's combined
// equation with the key terms collapsed per key.  With k(i) the key index of item i and S_k = sum_{i: k(i) = k} z_i c_i mod r,
//     sum_i z_i (u_i G + c_i PK_k(i) - R_i)  =  (sum_i z_i u_i) G  +  sum_k S_k PK_k  -  sum_i z_i R_i
// (the double scheme's second equation with z'_i, G', PK'_k, R'_i; the per-item generator's u_i Gen_k(i) collapses the same way
// with T_k = sum z_i u_i).  The steps, each a function here that the device runs one lane per unit and the CPU build in a loop:
//   item     ksv_item: prepare_item in keyed mode with the R point(s) given their own residue test and no equation; the key's
//            flags fail the item (the keys had their tests when the set was built); z_i on -R_i goes to the MSM (msm.h, with
//            the windows the short weights reach: msm_short_windows), a_i = z_i c_i (and z'_i c_i, or z_i u_i) to the
//            per-item scalar column of the key's point column;
//   runs     the items grouped by key (the counting sort of the key-set's large variant), then a key's run summed mod r in
//            pieces: the sorted positions are ruled off every KSV_PIECE; a key's lane sums its run up to the first line
//            (ksv_head), a line's lane sums from the line to the next line or the end of the run that crosses it (ksv_cell).
//            A run of any length is so cut into pieces of at most KSV_PIECE items, and a batch on one key costs what a
//            spread-out batch costs;
//   keys     ksv_key_point: S_k = head + the cells of the run, then S_k * PK_k over the set's window tables (kt_add_scalar:
//            one addition per position).  A key with an empty run, a zero sum or a point that is not valid is skipped: an
//            invalid key has no tables, and its items have failed the batch in the item pass;
//   verdict  the key points and the MSM total added, bv_verdict.
// Soundness: the collapse is an identity in the group, so the sum is the same element as batch_verdict.h's, and its argument
// carries over: every R is tested point by point, every key that contributes was found torsion-free at registration, hence
// every D_i = u_i G + c_i PK_k(i) - R_i has order 1 or r, and for any values of the other weights at most one z_j cancels a
// D_j != O.  Two bad items under the SAME key are no exception: their defects meet in S_k, but z_1 and z_2 are drawn
// independently, so z_1 D_1 + z_2 D_2 = O for at most one z_2 given z_1: probability <= 2^-128.
#pragma once
#include "batch_verdict.h"
#include "keyset.h"

namespace jjs {

constexpr uint32_t KSV_PIECE = 512;          // items per piece of a run

struct ksv_params {
    verify_params V;             // the scheme's descriptor with the key columns gathered per item (ks_index_item), key_flag
                                 // non-zero (keyed mode) and pre_malformed = the index pass's flags
    uint32_t seed[8];
    int z_bits;                  // bits of the weights (msm_weight_bits)
    uint32_t n_cols;             // point columns of the set: 1 single, 2 double (PK, PK') and per-item generator (PK, Gen)
    const uint32_t* keyid;       // [n] the clamped key index of an item
    const uint8_t* key_flags[2]; // [n_keys] KT_KEY_* of each point column
    uint32_t* terms;             // n_eq * n cached addends: R, then R'
    uint8_t* scalars;            // n_eq * n weights, 32 bytes each
    uint8_t* a[2];               // [n] x 32 bytes: the item's scalar on its key's point of column 0 / 1
    uint32_t* fail;              // non-zero: some item failed a per-item check
    uint8_t* partial;            // per block of the pass: sum z u, sum z' u mod r (64 bytes)
};

// both point columns of the item's key are valid (and so have tables)
JJS_HD bool ksv_key_ok(const ksv_params& B, uint32_t id) {
    uint32_t f = B.key_flags[0][id];
    if (B.n_cols > 1) f = (f & B.key_flags[1][id] & KT_KEY_VALID) | ((f | B.key_flags[1][id]) & KT_KEY_MALFORMED);
    return (f & KT_KEY_VALID) != 0 && (f & KT_KEY_MALFORMED) == 0;
}

// One item: the checks, the R term(s), the scalars on the key's points, and z u (z' u) mod r for the fixed generator(s).
// Returns false when the item fails a check; its weights are then zero.
JJS_HD bool ksv_item(const ksv_params& B, uint64_t item, words8 zu[2]) {
    verify_params P = B.V;
    const uint64_t n = P.n;
    P.n_eq = 0;                                                         // no Euclid, no combined test
    P.own_test_mask = ((1u << P.n_points) - 1u) & ~P.key_points_mask;   // R (R'): their own residue test; the keys had theirs
    P.c_out = nullptr; P.small_mode = 0;
    const prep_record r = prepare_item(P, item, false);
    const bool ok = !r.malformed && r.valid && ksv_key_ok(B, B.keyid[item]);
    words8 z[2];
    bv_weights(B.seed, item, B.z_bits, z[0], z[1]);
    const words8 u = load_words(B.V.u, item);
    zu[0] = words_zero(); zu[1] = words_zero();
    for (uint32_t e = 0; e < B.V.n_eq; ++e) {
        const words8 w = select_words(ok, z[e], words_zero());
        const eq_desc& E = B.V.eq[e];
        msm_store_term(B.terms + (e * n + item) * MSM_TERM_WORDS, load_fq(E.r, item), load_fq(E.r, item, 32));
        store_words(B.scalars, e * n + item, w);
        store_words(E.pk_col ? B.a[1] : B.a[0], item, fr_mul(w, r.c));
        const words8 wu = ok ? fr_mul(w, u) : words_zero();
        if (E.comb) zu[e] = wu;
        else store_words(E.gen_col ? B.a[1] : B.a[0], item, wu);
    }
    return ok;
}

// ---- the runs ---------------------------------------------------------------------------------------------------------------
// cursor: the counting sort's cursors after the scatter, cursor[k * stride] = the end of key k's run (the start of k + 1's)
struct ksv_runs {
    const uint32_t* cursor;
    uint32_t stride;
    const uint32_t* order;       // [n] the items in key order
    const uint32_t* keyid;       // [n]
    uint32_t n_keys;
    uint64_t n;
};
JJS_HD uint32_t ksv_run_start(const ksv_runs& R, uint32_t k) { return k ? R.cursor[(size_t)(k - 1) * R.stride] : 0u; }
JJS_HD uint32_t ksv_run_end(const ksv_runs& R, uint32_t k) { return R.cursor[(size_t)k * R.stride]; }
JJS_HD uint32_t ksv_cells(uint64_t n) { return (uint32_t)((n + KSV_PIECE - 1) / KSV_PIECE); }
JJS_HD words8 ksv_sum(const ksv_runs& R, const uint8_t* a, uint32_t lo, uint32_t hi) {
    words8 acc = words_zero();
    for (uint32_t p = lo; p < hi; ++p) acc = fr_add(acc, load_words(fe_src{a, 32, 0}, R.order[p]));
    return acc;
}
// key k's run from its start to the first line at or behind it (nothing when the run starts on a line)
JJS_HD words8 ksv_head(const ksv_runs& R, const uint8_t* a, uint32_t k) {
    const uint32_t lo = ksv_run_start(R, k), end = ksv_run_end(R, k);
    const uint32_t line = (lo + KSV_PIECE - 1) / KSV_PIECE * KSV_PIECE;
    return ksv_sum(R, a, lo, line < end ? line : end);
}
// line g (position g * KSV_PIECE < n): from the line to the next one or to the end of the run the line falls in
JJS_HD words8 ksv_cell(const ksv_runs& R, const uint8_t* a, uint32_t g) {
    const uint32_t lo = g * KSV_PIECE, end = ksv_run_end(R, R.keyid[R.order[lo]]);
    return ksv_sum(R, a, lo, lo + KSV_PIECE < end ? lo + KSV_PIECE : end);
}
// S_k from the heads and the cells: the lines inside the run [start, end) are ceil(start / PIECE) .. ceil(end / PIECE) - 1
JJS_HD words8 ksv_key_sum(const ksv_runs& R, const uint8_t* head, const uint8_t* cell, uint32_t k) {
    const uint32_t lo = ksv_run_start(R, k), end = ksv_run_end(R, k);
    words8 acc = load_words(fe_src{head, 32, 0}, k);
    for (uint32_t g = (lo + KSV_PIECE - 1) / KSV_PIECE; g < (end + KSV_PIECE - 1) / KSV_PIECE; ++g)
        acc = fr_add(acc, load_words(fe_src{cell, 32, 0}, g));
    return acc;
}
JJS_HD bool words_is_zero(const words8& a) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v |= a.w[i];
    return v == 0;
}
// S_k * P_k for key k of point column C
JJS_HD ext_pt ksv_key_point(const ksv_runs& R, const key_column& C, const uint8_t* head, const uint8_t* cell, uint32_t k) {
    if (ksv_run_start(R, k) == ksv_run_end(R, k)) return ext_identity();
    if ((C.key_flags[k] & (KT_KEY_VALID | KT_KEY_MALFORMED)) != KT_KEY_VALID) return ext_identity();    // no tables: never read
    const words8 S = ksv_key_sum(R, head, cell, k);
    if (words_is_zero(S)) return ext_identity();
    return kt_add_scalar(ext_identity(), C, k, S, KEYSET_WINDOW);
}

}  // namespace jjs

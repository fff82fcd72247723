// The verifier's half of the multisignature scheme (include/jjs_gpu.h jjs_multisig_aggregate_pk*, jjs_multisig_verify*):
//   aggregate_pk          reference src/multisig.rs:154-156, 416-429   pk_agg = sum d_i * PK_i, d_i = H(pk_i, pk_1 .. pk_n)
//   PublicKey::verify     on (u, R, pk_agg, m): the resident single-scheme call, unchanged
// over many key vectors at once, vector t owning rows [offsets[t], offsets[t+1]) of the key column.  A verifier holds no
// shares, so only the two front passes of multisig_core.h run; the passes:
//   0   msig_map_item                                                   lane per vector      (unchanged)
//   c   mv_check_item: range and on-curve test of every key, the vector of an unusable key marked refused   lane per key row
//       (the key-set form runs mk_gather_item of msig_keyset.h instead: a registered valid key is canonical and on the curve)
//   1   msig_delin_item / mk_delin_item                                 lane (or eight) per key row   (unchanged)
//   s   mv_sum_item: pk_agg = sum D_i, normalised and stored; vec_status; what a refused vector gets   lane per vector
//   v   the single-scheme verification on (u, R, agg_pk, m)             (the verification calls only)
//   z   mv_clear_item: agg_pk of a refused vector zeroed                lane per vector      (the verification calls only)
// The sum pass runs no binding hash (msig_agg_item computes `a`, which a verifier does not need).  An empty vector is
// usable: aggregate_pk(&[]) is the identity, (0, 1).  In a verification call the sum pass gives a refused vector an
// aggregate of 64 bytes of 0xFF: the range test of the verification turns it into status 3 and counts it in the tally, so
// nothing is patched behind the verification but the aggregate itself.
#pragma once
#include "multisig_core.h"
#include "msig_keyset.h"

namespace jjs {

struct msig_verify_params {
    msig_params M;               // PK, offsets, tr_of, d_words, dpk, tags, long_tags, lane_ws, agg_pk; nothing else is read
    uint32_t* refused;           // scratch: [B] non-zero: the vector holds an unusable key (cleared by the call)
    uint8_t* vec_status;         // [B] 0 usable / 3 refused; nullable
    uint32_t poison, pad_;       // what the sum pass stores for a refused vector: 0 zeros, 1 64 bytes of 0xFF
};
struct msig_verify_keyset_params {
    msig_keyset_params K;        // K.M.PK is the gathered column; K.refused is the refused word of every vector
    uint8_t* vec_status;
    uint32_t poison, pad_;
};
JJS_HD msig_verify_params mv_of(const msig_verify_keyset_params& V) {
    msig_verify_params P{};
    P.M = V.K.M; P.refused = V.K.refused; P.vec_status = V.vec_status; P.poison = V.poison;
    return P;
}

// a key as the calls accept it: both coordinates canonical, and on the curve
JJS_HD bool mv_key_usable(const words8& u, const words8& v) {
    if (!words_lt(u, JJS_Q_WORDS) || !words_lt(v, JJS_Q_WORDS)) return false;
    return affine_on_curve(fq_from_words(u), fq_from_words(v));
}
// the check pass (lane per key row, behind pass 0)
JJS_HD void mv_check_item(const msig_verify_params& V, uint64_t i) {
    const fe_src pk{V.M.PK, 64, 0};
    if (!mv_key_usable(load_words(pk, i), load_words(pk, i, 32))) V.refused[V.M.tr_of[i]] = 1u;   // a plain store: every writer stores the same word
}
// the sum pass (lane per vector)
JJS_HD void mv_sum_item(const msig_verify_params& V, uint32_t t) {
    const msig_params& P = V.M;
    const bool refused = V.refused[t] != 0;
    if (V.vec_status) V.vec_status[t] = (uint8_t)(refused ? (uint32_t)ST_MALFORMED : (uint32_t)ST_OK);
    if (refused) {
        words8 fill;
        for (int k = 0; k < 8; ++k) fill.w[k] = V.poison ? 0xFFFFFFFFu : 0u;
        store_words(P.agg_pk, 2 * (uint64_t)t, fill);
        store_words(P.agg_pk, 2 * (uint64_t)t + 1, fill);
        return;
    }
    store_point(P.agg_pk, t, sum_points_affine(P.dpk, P.offsets[t], P.offsets[t + 1]));      // no rows: the identity, (0, 1)
}
// the clear pass (lane per vector, behind the verification)
JJS_HD void mv_clear_item(const msig_verify_params& V, uint32_t t) {
    if (!V.refused[t]) return;
    store_words(V.M.agg_pk, 2 * (uint64_t)t, small_words(0));
    store_words(V.M.agg_pk, 2 * (uint64_t)t + 1, small_words(0));
}

}  // namespace jjs

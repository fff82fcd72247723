// Registered key sets (include/jjs_gpu.h jjs_keyset_*): the key-table path of key_tables.h with tables that outlive the call.
//
// A caller that knows its keys ahead of time (a validator set, a wallet's accounts, the signers of a contract) registers
// them once: every key is decoded or normalised, gets its `is_valid` test, its chain of bases and its window tables
// {0 .. 2^(w-1)} * 2^(w i) * PK (w = KEYSET_WINDOW), all on the device, kept until the set is destroyed.  A call then carries
// a 4-byte index per item instead of the key, and no dedup, decision, chain or table kernel runs per call:
//   index    clamp key_idx[i] to the set (an index beyond it makes the item malformed), the dense key id of the item, and its
//            key point(s) gathered into a per-item column for the challenge hash (ks_index_item);
//   large    (more than KEYSET_SMALL_MAX_ITEMS items) the items grouped by key with the key-table path's counting sort, the
//            hashes in keyed mode, then kt_finish_item with a key_params whose columns point into the set: one lane per item;
//   small    (at most KEYSET_SMALL_MAX_ITEMS) the hash on eight lanes per item, then `positions` adjacent lanes per equation,
//            lane k adding the digits k, k + positions, ... of c over the key's tables and its share of the comb digits of u*G
//            (or of u's digits over Gen's tables), the partial sums added across the lanes (ks_piece): no Euclid step and no
//            chain on the critical path, which is the hash.
// Statuses: those of the existing entry point given the key inline, with the key's own flags folded in (Malformed >
// InvalidPoint > InvalidSignature); an item whose equation fails goes to the resolve pass for R's subgroup test as on the
// key-table path.
#pragma once
#include "key_tables.h"

namespace jjs {

constexpr int KEYSET_WINDOW = KT_WINDOW_WIDE;        // 43 positions x 33 entries x 144 B = 204 KB of tables per key point
constexpr uint64_t KEYSET_SMALL_MAX_ITEMS = 16384;
constexpr uint32_t KEYSET_MAX_KEYS = 1u << 24;

// status of a registered key from the flags of its points (kt_key_flags, plus KT_KEY_MALFORMED for an encoding that did
// not decode or normalise): the worse of the points wins
JJS_HD uint32_t ks_key_status(uint32_t f0, uint32_t f1) {
    if ((f0 | f1) & KT_KEY_MALFORMED) return ST_MALFORMED;
    return ((f0 & f1) & KT_KEY_VALID) ? ST_OK : ST_INVALID_POINT;
}

// Positions of the latency variant by call size: finer pieces for the smaller calls, where the chip has lanes to spare.
JJS_HD uint32_t ks_small_positions(uint64_t n) { return n <= 2048 ? 16u : (n <= 8192 ? 8u : 4u); }

// The index pass of one item: the clamped key id, the item's malformed flag for an index outside the set, and the key
// point(s) copied to the item's row of the gathered columns (`n_cols` of them; keys[c] holds n_keys x 64 affine bytes).
JJS_HD void ks_index_item(const uint32_t* key_idx, uint32_t n_keys, uint64_t item, uint32_t* keyid, uint8_t* bad,
                          uint32_t n_cols, const uint8_t* keys0, const uint8_t* keys1, uint8_t* out0, uint8_t* out1) {
    const uint32_t idx = key_idx[item];
    const bool in_set = idx < n_keys;
    const uint32_t id = in_set ? idx : 0u;
    keyid[item] = id;
    if (!in_set) bad[item] = 1;
    const fe_src k0{keys0, 64, 0};
    store_words(out0, 2 * item, load_words(k0, id));
    store_words(out0, 2 * item + 1, load_words(k0, id, 32));
    if (n_cols > 1) {
        const fe_src k1{keys1, 64, 0};
        store_words(out1, 2 * item, load_words(k1, id));
        store_words(out1, 2 * item + 1, load_words(k1, id, 32));
    }
}

// Lane k of `positions` lanes of equation e of one item (latency variant): digits k, k + positions, ... of c over the
// key's tables, plus comb digits [k * COMB_WINDOWS / positions, (k + 1) * ...) of u*G (fixed generator) or digits k,
// k + positions, ... of u over the generator's tables.  T of the result is valid (the pieces are added across lanes).
JJS_HD ext_pt ks_piece(const verify_params& P, const key_params& K, uint64_t item, uint32_t e, uint32_t k, uint32_t positions,
                       const prep_record& r) {
    const int w = KEYSET_WINDOW;
    const eq_desc& E = P.eq[e];
    const words8 u = load_words(P.u, item);
    ext_pt acc = ext_identity();
    const key_column C = kt_col(K, E.pk_col);
    const uint32_t id = C.keyid[item];
    const words8 sc = kt_recode(r.c, w);
    for (int pos = (int)k; pos < kt_positions(w); pos += (int)positions)
        acc = kt_add_digit(acc, kt_table(C, id, (uint32_t)pos, w), sc, pos, w);
    if (E.comb) {
        const int per = COMB_WINDOWS / (int)positions;
        return add_comb_range(acc, E.comb, u, per * (int)k, per * (int)k + per, true);
    }
    const key_column G = kt_col(K, E.gen_col);
    const words8 su = kt_recode(u, w);
    for (int pos = (int)k; pos < kt_positions(w); pos += (int)positions)
        acc = kt_add_digit(acc, kt_table(G, id, (uint32_t)pos, w), su, pos, w);
    return acc;
}
// the verdict of an item of the latency variant from its equations' sums; the precedence of kt_finish_item
JJS_HD uint32_t ks_small_status(const verify_params& P, const key_params& K, uint64_t item, const prep_record& r, bool eq_ok) {
    bool keys_valid = true, keys_malformed = false;
    const uint32_t id = K.col[0].keyid[item];
    for (uint32_t c = 0; c < K.n_cols; ++c) {
        const uint32_t f = (c == 0 ? K.col[0].key_flags : K.col[1].key_flags)[id];
        keys_valid = keys_valid && (f & KT_KEY_VALID) != 0;
        keys_malformed = keys_malformed || (f & KT_KEY_MALFORMED) != 0;
    }
    if (r.malformed || keys_malformed || !words_lt(load_words(P.u, item), JJS_FR_WORDS)) return ST_MALFORMED;
    if (!r.valid || !keys_valid) return ST_INVALID_POINT;
    return eq_ok ? ST_OK : ST_PENDING_EQ_FAILED;
}
JJS_HD bool ks_equation_holds(const verify_params& P, uint64_t item, uint32_t e, const ext_pt& total) {
    return ext_eq_affine(total, load_fq(P.eq[e].r, item), load_fq(P.eq[e].r, item, 32));
}

// The latency variant of one item on one thread: the CPU build's reference run of the device's lanes, the partial sums
// added in the order of the device's shuffle tree (lane ^ 1, ^ 2, ^ 4, ^ 8).
JJS_HD uint32_t ks_small_item_serial(const verify_params& P, const key_params& K, uint64_t item, uint32_t positions,
                                     const prep_record& r) {
    bool eq_ok = true;
    for (uint32_t e = 0; e < P.n_eq; ++e) {
        ext_pt part[16];
        for (uint32_t k = 0; k < positions; ++k) part[k] = ks_piece(P, K, item, e, k, positions, r);
        for (uint32_t step = 1; step < positions; step <<= 1)
            for (uint32_t k = 0; k < positions; k += 2 * step) part[k] = ext_add_niels(part[k], to_niels(part[k + step]), false, true);
        eq_ok = ks_equation_holds(P, item, e, part[0]) && eq_ok;
    }
    return ks_small_status(P, K, item, r, eq_ok);
}

}  // namespace jjs

// Adding keys to a live key set (include/jjs_gpu.h jjs_keyset_add, jjs_keyset_reserve): the plan that says which of the offered
// keys are new, and where each of them goes.  Every function here is JJS_HD: the device runs them in the keyset_add_*_kernel
// family (keyset_add_kernels.h), the CPU build in tests/hostbuild/keyset_add_harness.cpp.
//
// The candidates arrive as the canonical affine rows jjs_keyset_create would store for them (64 bytes per point column: copied,
// normalised or decoded by the kernels create uses) and a `bad` byte per candidate (an encoding that did not decode or
// normalise).  JJS_KEYSET_ADD_UNIQUE then runs four steps, one lane per candidate, 16-byte row loads, nothing per lane in scratch:
//   probe    a candidate that is `bad` or has a coordinate >= q is MALFORMED: it has no canonical row, nothing could ever find it,
//            and it is not registered.  Every other candidate's row is probed in the set's lookup table (kl_find_affine): a hit is
//            the (lowest) index jjs_keyset_find would report, and nothing is registered for it.
//   claim    the misses are entered into a scratch lookup table whose KEYS ARE THE CANDIDATE ROWS (kl_insert; the hits and the
//            malformed candidates carry KT_KEY_MALFORMED in its flags, so they are not entered): equal candidates share one slot,
//            which ends up holding the LOWEST position among them whatever the order the lanes ran in.
//   scan     a miss that finds its own position in the scratch table is a first occurrence; an exclusive scan over those flags
//            gives its rank.  The scan spans blocks: BLOCK candidates per block are counted (ka_mark + the block's count), the
//            block counts are scanned by one block of KA_SCAN_LANES lanes, lane j taking ka_scan_chunk(blocks) consecutive
//            counts (two passes over its chunk around a scan of the lanes' totals), and the gather adds the rank inside the
//            block.  Its edges are a multiple of BLOCK candidates and KA_SCAN_LANES blocks (65 536 candidates: one count per lane).
//   gather   a first occurrence's rows go to row n_old + rank of the set; every candidate learns its index: the hit, n_old + the
//            rank of the first occurrence of its row, or KA_MALFORMED.
// Indices are therefore a function of the input alone, never of the order the lanes ran in.  JJS_KEYSET_ADD_APPEND skips all of
// this: candidate i goes to n_old + i, whatever it is.
//
// Both modes then run key_chain_kernel / keyset_flags_kernel / key_table_kernel over the new range only, through a key_params
// whose columns START AT n_old, and enter the new ids into the set's lookup table (kl_insert with global ids).
//
// WHY THE LIVE TABLE MAY BE EXTENDED IN PLACE.  Launches of the old set may probe the table while the new ids are entered.  That
// is safe because of two properties of keyset_lookup.h, which every change to it must keep:
//   - a probe SKIPS a slot whose id is >= its own n_keys (kl_find_*: `c < T.n_keys`): a launch that was queued against n_old keys
//     walks past every new id as if the slot were taken by a stranger, and still ends at an empty slot;
//   - equal keys only ever LOWER a slot (atomicMin), and a new id is larger than every old one: no slot an old launch can hit
//     changes its value.
// A table with more slots is built beside the live one, never over it (keyset_add_calls.h: every slot count has its own region).
#pragma once
#include "keyset.h"
#include "keyset_lookup.h"

namespace jjs {

constexpr uint32_t KA_MALFORMED = 0xFFFFFFFFu;     // the index of a candidate that was not registered (idx_out)
constexpr uint32_t KA_NEW = 0xFFFFFFFEu;           // probe result: not in the set (never leaves the plan)
constexpr uint32_t KA_RETRACTED = 0xFFFFFFFDu;     // a slot of the live table whose id a failed add had entered: taken, and never a hit
constexpr uint32_t KA_SCAN_LANES = 256;            // lanes of the one block that scans the block counts

struct keyset_add_plan {
    keyset_lookup S;          // the set as it is: its rows, flags and lookup table over n_old keys
    keyset_lookup C;          // the scratch table: keys = the candidate rows, flags = `skip` (both columns), n_keys = n
    const uint8_t* bad;       // [n] the candidate's encoding did not decode / normalise
    uint8_t* skip;            // [n] KT_KEY_MALFORMED: takes no part in the claim (malformed, or already in the set)
    uint32_t* res;            // [n] probe: the index it was found at, KA_NEW or KA_MALFORMED
    uint32_t* lead;           // [n] a new candidate: the position of the first occurrence of its row
    uint8_t* first;           // [n] 1: a first occurrence
    uint32_t* sums;           // [blocks + 1] first occurrences per block of BLOCK candidates -> their exclusive scan, then the total
    uint32_t* rank;           // [n] a first occurrence: its rank among them
    uint8_t* dst[2];          // the set's rows FROM n_old ON, per point column
    uint32_t n, n_old;
};

JJS_HD bool ka_row_canonical(const keyset_lookup& T, const kl_key& k) {
    bool ok = words_lt(k.u[0], JJS_Q_WORDS) && words_lt(k.v[0], JJS_Q_WORDS);
    if (T.n_cols > 1) ok = ok && words_lt(k.u[1], JJS_Q_WORDS) && words_lt(k.v[1], JJS_Q_WORDS);
    return ok;
}

// probe, one lane per candidate
JJS_HD void ka_probe(const keyset_add_plan& P, uint32_t i) {
    const kl_key k = kl_load_row(P.C, i);
    uint32_t r = KA_MALFORMED;
    if (!P.bad[i] && ka_row_canonical(P.C, k)) {
        const uint32_t hit = kl_find_affine(P.S, k);
        r = hit == KL_MISS ? KA_NEW : hit;
    }
    P.res[i] = r;
    P.skip[i] = r == KA_NEW ? 0 : (uint8_t)KT_KEY_MALFORMED;
}
// claim, one lane per candidate (the scratch table's slots arrive as KL_EMPTY)
JJS_HD void ka_claim(const keyset_add_plan& P, uint32_t i) { kl_insert(P.C, i); }
// behind the claim: is candidate i the first occurrence of its row?
JJS_HD uint32_t ka_mark(const keyset_add_plan& P, uint32_t i) {
    uint32_t f = 0;
    if (P.res[i] == KA_NEW) {
        const uint32_t lead = kl_find_affine(P.C, kl_load_row(P.C, i));
        P.lead[i] = lead;
        f = lead == i ? 1u : 0u;
    }
    P.first[i] = (uint8_t)f;
    return f;
}
// the scan of the block counts: lane j of KA_SCAN_LANES takes counts [j * chunk, (j + 1) * chunk)
JJS_HD uint32_t ka_scan_chunk(uint32_t blocks) { return (blocks + KA_SCAN_LANES - 1) / KA_SCAN_LANES; }
JJS_HD uint32_t ka_scan_chunk_total(const uint32_t* sums, uint32_t blocks, uint32_t j) {
    const uint32_t chunk = ka_scan_chunk(blocks);
    uint32_t t = 0;
    for (uint64_t b = (uint64_t)j * chunk; b < (uint64_t)(j + 1) * chunk && b < blocks; ++b) t += sums[b];
    return t;
}
JJS_HD void ka_scan_chunk_write(uint32_t* sums, uint32_t blocks, uint32_t j, uint32_t base) {
    const uint32_t chunk = ka_scan_chunk(blocks);
    for (uint64_t b = (uint64_t)j * chunk; b < (uint64_t)(j + 1) * chunk && b < blocks; ++b) {
        const uint32_t c = sums[b];
        sums[b] = base;
        base += c;
    }
}
// gather: candidate i, a first occurrence of rank `rank`
JJS_HD void ka_gather(const keyset_add_plan& P, uint32_t i, uint32_t rank) {
    P.rank[i] = rank;
    for (uint32_t c = 0; c < P.C.n_cols; ++c) {
        const fe_src s{P.C.keys[c], 64, 0};
        store_words(P.dst[c], 2 * (uint64_t)rank, load_words(s, i));
        store_words(P.dst[c], 2 * (uint64_t)rank + 1, load_words(s, i, 32));
    }
}
// the index candidate i is answered with (behind the gather)
JJS_HD uint32_t ka_index(const keyset_add_plan& P, uint32_t i) {
    const uint32_t r = P.res[i];
    return r == KA_NEW ? P.n_old + P.rank[P.lead[i]] : r;
}
// ... and its key_status, from the flags of the set once the new range has them: what jjs_keyset_create reports for the key
JJS_HD uint32_t ka_status(uint32_t idx, uint32_t n_cols, const uint8_t* flags0, const uint8_t* flags1) {
    if (idx == KA_MALFORMED) return ST_MALFORMED;
    return ks_key_status(flags0[idx], n_cols > 1 ? flags1[idx] : (uint32_t)KT_KEY_VALID);
}

// An add in place that fails behind its lookup insert takes its ids out of the live table again: slot i, if it holds an id
// >= n_old, becomes KA_RETRACTED -- not KL_EMPTY, which would cut the probe sequences that pass through it.  Every probe and
// every insert walks past the value as past a stranger (it is neither KL_EMPTY nor < n_keys).  Left in, such an id could be met
// by a later key registered at the same index before that key's own slot, and hide a lower index of an equal key.
JJS_HD void ka_retract(uint32_t* slots, uint32_t i, uint32_t n_old) {
    const uint32_t c = slots[i];
    if (c != KL_EMPTY && c >= n_old) slots[i] = KA_RETRACTED;
}

}  // namespace jjs

// Removing keys from a live key set, and compacting it (include/jjs_gpu.h jjs_keyset_remove, jjs_keyset_compact).  Every
// function here is JJS_HD: the device runs them in the keyset_remove_*_kernel family (keyset_remove_kernels.h), the CPU build in
// tests/hostbuild/keyset_remove_harness.cpp.
//
// REMOVE makes index d behave as an index whose key was registered malformed.  It runs four steps behind one another:
//   answer   one lane per candidate: the key's status before the call from its flag bytes -- 0, 1 or 3, KR_WAS_REMOVED for a key
//            that carries KT_KEY_REMOVED, KR_NOT_IN_RANGE for an index >= n_keys, which addresses nothing from here on.
//   flags    one lane per candidate, in a launch behind the answers: KT_KEY_MALFORMED | KT_KEY_REMOVED set and KT_KEY_VALID
//            cleared in every point column's flag byte, by word atomics on the aligned word that holds the byte (the other three
//            bytes keep their bits).  The lane whose atomicOr on the first column finds KT_KEY_REMOVED clear is THE lane that
//            removed the index: it counts it, and counts it as valid when its answer was 0.  So the counts are of distinct
//            indices whatever the order the lanes ran in.  Every verifying kernel tests KT_KEY_VALID and KT_KEY_MALFORMED only.
//   retract  one lane per candidate whose answer was 0 or 1 (a key that is in the lookup table): it walks its own row's probe
//            sequence, and the slot that holds exactly this id becomes KA_RETRACTED -- never KL_EMPTY, which would cut the
//            sequences that pass through it.  A higher duplicate of a registered key is in no slot: its walk ends at an empty one.
//   re-enter one lane per id of the SET: an id that is neither removed nor malformed and whose own row kl_find_affine now
//            misses -- or finds at a HIGHER id: another duplicate's lane was here first -- was a higher duplicate of a retracted
//            id; it enters itself with kl_insert, ties settling on the lowest index by atomicMin whatever the order of the
//            lanes.  This restores "found at the lowest surviving index".
// Rows, tables and on-curve bytes are not written: a removed id is in no slot, so nothing reads its on-curve byte, and its
// flags keep every kernel from its tables.
//
// THE HALF-FULL BOUND (the third property every change must keep, beside the two keyset_add.h states).  Every taken slot,
// live or KA_RETRACTED, belongs to a distinct index of the set: a live slot to the id it holds, a retracted one to the removed id
// it held, and a removed id never enters again (kl_insert skips malformed keys; a re-registered equal key gets a NEW index).
// kl_slot_count is sized by n_keys, which counts removed indices, so at most half the slots are ever taken and every probe
// sequence ends at an empty slot -- except for the slots failed adds retract (keyset_add_calls.h), which were there before.
// A table built anew (an add that needs more slots, a moving add's rebuild, compact) starts from empty and skips removed ids.
//
// COMPACT gathers the survivors, in order, into a new allocation: mark (survivors per block of BLOCK ids), the add's scan over
// the block counts, a gather by ballot rank of rows, flag bytes, on-curve bytes, src[new id] = old id and map[old id] = new id,
// then the table gather (keyset_remove_kernels.h) and a lookup table built from empty over the new ids.
#pragma once
#include "keyset_add.h"

namespace jjs {

constexpr uint32_t KT_KEY_REMOVED = 4;             // beside KT_KEY_MALFORMED (1) and KT_KEY_VALID (2) in a key's flag byte
constexpr uint32_t KR_WAS_REMOVED = 8, KR_NOT_IN_RANGE = 0xFF;      // result[] of jjs_keyset_remove
constexpr uint32_t KR_GONE = 0xFFFFFFFFu;          // map_out[] of jjs_keyset_compact: a removed index
constexpr uint32_t KR_TABLE_SLICE = 1024;          // 16-byte units of a key's table one block of the table gather moves

struct keyset_remove_plan {
    keyset_lookup T;          // the live set: rows, flags, its lookup table, n_keys
    uint8_t* flags[2];        // the flag bytes, writable (T.flags, per point column; 4-byte aligned)
    const uint32_t* idx;      // [n] the candidates
    uint8_t* result;          // [n] the answers
    uint32_t* counts;         // [0] distinct indices removed by this call, [1] those among them whose status was 0
    uint32_t n;
};

// answer, one lane per candidate
JJS_HD void kr_answer(const keyset_remove_plan& P, uint32_t i) {
    const uint32_t id = P.idx[i];
    uint32_t r = KR_NOT_IN_RANGE;
    if (id < P.T.n_keys) {
        const uint32_t f0 = P.T.flags[0][id], f1 = P.T.n_cols > 1 ? (uint32_t)P.T.flags[1][id] : (uint32_t)KT_KEY_VALID;
        r = ((f0 | f1) & KT_KEY_REMOVED) ? KR_WAS_REMOVED : ks_key_status(f0, f1);
    }
    P.result[i] = (uint8_t)r;
}
// the flag byte `id` of a column through the aligned word that holds it; returns the byte as it was
JJS_HD uint32_t kr_mark_byte(uint8_t* flags, uint32_t id) {
    uint32_t* const word = reinterpret_cast<uint32_t*>(flags) + (id >> 2);
    const uint32_t shift = 8u * (id & 3u);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t was = atomicOr(word, (KT_KEY_MALFORMED | KT_KEY_REMOVED) << shift);
    atomicAnd(word, ~(KT_KEY_VALID << shift));
#else
    const uint32_t was = *word;
    *word = (was | ((KT_KEY_MALFORMED | KT_KEY_REMOVED) << shift)) & ~(KT_KEY_VALID << shift);
#endif
    return (was >> shift) & 0xFFu;
}
// flags, one lane per candidate (behind every answer)
JJS_HD void kr_flags(const keyset_remove_plan& P, uint32_t i) {
    const uint32_t id = P.idx[i];
    if (id >= P.T.n_keys) return;
    const uint32_t was = kr_mark_byte(P.flags[0], id);
    if (P.T.n_cols > 1) (void)kr_mark_byte(P.flags[1], id);
    if (was & KT_KEY_REMOVED) return;              // another lane, or an earlier call, removed it
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&P.counts[0], 1u);
    if (P.result[i] == ST_OK) atomicAdd(&P.counts[1], 1u);
#else
    P.counts[0] += 1u;
    if (P.result[i] == ST_OK) P.counts[1] += 1u;
#endif
}
// retract, one lane per candidate
JJS_HD void kr_retract(const keyset_remove_plan& P, uint32_t i) {
    if (P.result[i] > ST_INVALID_POINT) return;    // malformed before, removed before, out of range: in no slot
    const uint32_t id = P.idx[i];
    uint32_t slot = (uint32_t)kl_hash_affine(P.T, kl_load_row(P.T, id)) & P.T.mask;
    for (uint32_t probe = 0; probe <= P.T.mask; ++probe) {
        const uint32_t c = P.T.slots[slot];
        if (c == KL_EMPTY) return;
        if (c == id) { P.T.slots[slot] = KA_RETRACTED; return; }
        slot = (slot + 1u) & P.T.mask;
    }
}
// re-enter, one lane per id of the set (behind every retraction)
JJS_HD void kr_reenter(const keyset_lookup& T, uint32_t id) {
    const uint32_t f = T.flags[0][id] | (T.n_cols > 1 ? (uint32_t)T.flags[1][id] : 0u);
    if (f & (KT_KEY_MALFORMED | KT_KEY_REMOVED)) return;
    if (kl_find_affine(T, kl_load_row(T, id)) > id) kl_insert(T, id);          // (KL_MISS is above every id)
}

// A by-key item whose probe found an index that a remove has flagged since (the probe ran ahead of the retraction): a miss, as
// kl_take_miss makes one -- the status the run left behind leaves the tally, KL_STATUS_NOT_IN_SET takes its place.  With a
// status column only: without one the run's status is not known, and the item stays what the by-index call makes of it.
JJS_HD bool kr_take_removed(const uint32_t* found, uint64_t item, uint32_t n_keys, const uint8_t* flags0, uint8_t* status, uint32_t* was) {
    const uint32_t c = found[item];
    if (!status || c >= n_keys || !(flags0[c] & KT_KEY_REMOVED)) return false;
    *was = status[item];
    status[item] = (uint8_t)KL_STATUS_NOT_IN_SET;
    return true;
}

// ---- compact ---------------------------------------------------------------------------------------------------------------------
struct keyset_compact_plan {
    const uint8_t* keys[2];   // the old set: rows, flags, on-curve bytes
    const uint8_t* flags[2];
    const uint8_t* on_curve;
    uint8_t* new_keys[2];     // the new one
    uint8_t* new_flags[2];
    uint8_t* new_on_curve;
    uint32_t* sums;           // [blocks + 1] survivors per block of BLOCK ids -> their exclusive scan, then the total
    uint32_t* src;            // [survivors] the old id of a new one
    uint32_t* map;            // [n_keys] the new id of an old one, or KR_GONE
    uint32_t n_keys, n_cols;
};
JJS_HD uint32_t kc_survives(const keyset_compact_plan& P, uint32_t id) { return (P.flags[0][id] & KT_KEY_REMOVED) ? 0u : 1u; }
// gather: old id `id`, a survivor of rank `rank`
JJS_HD void kc_gather(const keyset_compact_plan& P, uint32_t id, uint32_t rank) {
    for (uint32_t c = 0; c < P.n_cols; ++c) {
        const fe_src s{P.keys[c], 64, 0};
        store_words(P.new_keys[c], 2 * (uint64_t)rank, load_words(s, id));
        store_words(P.new_keys[c], 2 * (uint64_t)rank + 1, load_words(s, id, 32));
        P.new_flags[c][rank] = P.flags[c][id];
    }
    P.new_on_curve[rank] = P.on_curve[id];
    P.src[rank] = id;
    P.map[id] = rank;
}
// The table gather: block (new id, slice) moves 16-byte units [slice * KR_TABLE_SLICE, ...) of the key's `units` from the old
// id's table to the new one's; lane `lane` of `lanes` takes units lane, lane + lanes, ... of the slice.
struct keyset_table_gather {
    const uint32_t* old_tables[2];
    uint32_t* new_tables[2];
    const uint32_t* src;      // [n_new]
    uint32_t n_new, n_cols;
    uint32_t units;           // 16-byte units of one key's tables in one column
    uint32_t slices;          // ceil(units / KR_TABLE_SLICE)
};
typedef uint32_t kr_unit __attribute__((vector_size(16)));       // 16 bytes, moved by one load and one store
JJS_HD void kc_table_piece(const keyset_table_gather& G, uint64_t block, uint32_t lane, uint32_t lanes) {
    const uint32_t slice = (uint32_t)(block % G.slices);
    const uint64_t key = block / G.slices;
    const uint32_t col = (uint32_t)(key / G.n_new), id = (uint32_t)(key % G.n_new);
    if (col >= G.n_cols) return;
    const kr_unit* __restrict__ from = reinterpret_cast<const kr_unit*>(G.old_tables[col]) + (uint64_t)G.src[id] * G.units;
    kr_unit* __restrict__ to = reinterpret_cast<kr_unit*>(G.new_tables[col]) + (uint64_t)id * G.units;
    const uint32_t first = slice * KR_TABLE_SLICE, end = first + KR_TABLE_SLICE < G.units ? first + KR_TABLE_SLICE : G.units;
    // four loads in flight per lane, then their stores: adjacent lanes, adjacent units, on both sides
    // (a vector type in named values: an array of structs under conditions ended up in LDS)
    for (uint32_t u = first + lane; u < end; u += 4 * lanes) {
        if (u + 3 * lanes < end) {
            const kr_unit a = from[u], b = from[u + lanes], c = from[u + 2 * lanes], d = from[u + 3 * lanes];
            to[u] = a; to[u + lanes] = b; to[u + 2 * lanes] = c; to[u + 3 * lanes] = d;
        } else {                                   // the key's last slice
            for (uint32_t t = u; t < end; t += lanes) to[t] = from[t];
        }
    }
}

}  // namespace jjs

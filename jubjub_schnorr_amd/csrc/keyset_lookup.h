// Registered key sets by key (include/jjs_gpu.h jjs_keyset_find*, jjs_keyset_verify_keys*): the lookup table of a set and its
// probe.  Every function here is JJS_HD: the device runs them in keyset_lookup_insert_kernel / keyset_probe_kernel
// (device_kernels.h), the CPU build in tests/hostbuild/keyset_lookup_harness.cpp.
//
// The table is open addressing with linear probing over uint32_t slots, KL_EMPTY = 0xFFFFFFFF: kl_slot_count(n_keys) slots,
// the power of two >= 2 * n_keys and at least 8, so a probe always ends at an empty slot.  It lies in the set's one allocation.
//   hash     kt_hash's mixing (key_tables.h) over the ENCODING WORDS of the key's point column(s): 8 words per point, v with
//            bit 255 replaced by the parity of u -- what jjs_compress_dev writes for a canonical point.  A wire query is
//            hashed as it arrives (no square root), an affine one after two loads per point.
//   entered  every key whose flags do not carry KT_KEY_MALFORMED (such a key has no canonical bytes and never matches); keys
//            that are not `is_valid` ARE entered: an item naming one gets status 1, as inline.
//   ties     equal keys registered at several indices share one slot, which holds the LOWEST index whatever the order of
//            insertion: the first of them claims the empty slot (atomicCAS), every other meets it there -- equal keys share a
//            probe sequence and nothing is ever deleted -- and lowers it (atomicMin).
//   hits     decided by byte comparison with the set's affine rows, never by the hash: the 64 (128) affine bytes for an affine
//            query; for a wire query the 32 bytes per point against (v, parity of u) of the row, and only a row whose points
//            are ON THE CURVE may be hit (kl_on_curve, kept at registration).  An encoding that decodes is canonical, so for
//            such rows byte equality is "decodes to the registered point"; a registered off-curve key's would-be compression
//            decodes to another point or to none, and must miss as jjs_decompress_dev followed by the affine probe would.
#pragma once
#include "key_tables.h"

namespace jjs {

constexpr uint32_t KL_EMPTY = 0xFFFFFFFFu, KL_MISS = 0xFFFFFFFFu;
constexpr uint32_t KL_MIN_SLOTS = 8;

JJS_HD constexpr uint32_t kl_slot_count(uint32_t n_keys) {
    uint32_t s = KL_MIN_SLOTS;
    while (s < 2u * n_keys) s <<= 1;          // n_keys <= 2^24 (KEYSET_MAX_KEYS)
    return s;
}

struct keyset_lookup {
    const uint8_t* keys[2];     // the set's affine keys, n_keys x 64 per point column
    const uint8_t* flags[2];    // KT_KEY_* per point column
    uint8_t* on_curve;          // [n_keys] non-zero: every point of the key satisfies the curve equation (kl_insert writes it)
    uint32_t* slots;            // [mask + 1]
    uint32_t mask;
    uint32_t n_keys, n_cols;
    uint64_t seed;              // one per set
};

// the encoding words of an affine point: v, bit 255 replaced by the parity of u
JJS_HD words8 kl_encoding(const words8& u, const words8& v) {
    words8 r = v;
    r.w[7] = (v.w[7] & 0x7fffffffu) | ((u.w[0] & 1u) << 31);
    return r;
}
JJS_HD uint64_t kl_mix(uint64_t h, const words8& w) {
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        h ^= ((uint64_t)w.w[i + 1] << 32) | w.w[i];
        h *= 0xff51afd7ed558ccdull;
        h ^= h >> 29;
    }
    return h;
}
JJS_HD uint64_t kl_hash(const words8& e0, const words8& e1, uint32_t n_cols, uint64_t seed) {
    uint64_t h = kl_mix(0x9e3779b97f4a7c15ull ^ seed, e0);
    if (n_cols > 1) h = kl_mix(h, e1);
    return h;
}
JJS_HD uint32_t kl_diff(const words8& a, const words8& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d |= a.w[i] ^ b.w[i];
    return d;
}

// one key's point(s) or one query, in registers: u, v per point column (a wire query: `v` holds the encoding, `u` is unused)
struct kl_key {
    words8 u[2], v[2];
};
JJS_HD kl_key kl_load_row(const keyset_lookup& T, uint32_t id) {
    kl_key k{};
    const fe_src s0{T.keys[0], 64, 0};
    k.u[0] = load_words(s0, id); k.v[0] = load_words(s0, id, 32);
    if (T.n_cols > 1) {
        const fe_src s1{T.keys[1], 64, 0};
        k.u[1] = load_words(s1, id); k.v[1] = load_words(s1, id, 32);
    }
    return k;
}
JJS_HD uint64_t kl_hash_affine(const keyset_lookup& T, const kl_key& k) {
    return kl_hash(kl_encoding(k.u[0], k.v[0]), kl_encoding(k.u[1], k.v[1]), T.n_cols, T.seed);
}
JJS_HD bool kl_same_affine(const keyset_lookup& T, const kl_key& a, const kl_key& b) {
    uint32_t d = kl_diff(a.u[0], b.u[0]) | kl_diff(a.v[0], b.v[0]);
    if (T.n_cols > 1) d |= kl_diff(a.u[1], b.u[1]) | kl_diff(a.v[1], b.v[1]);
    return d == 0;
}

// Registration, one lane per key: the key's on-curve byte, and its entry unless the key is malformed.
JJS_HD void kl_insert(const keyset_lookup& T, uint32_t id) {
    const bool malformed = ((T.flags[0][id] | (T.n_cols > 1 ? T.flags[1][id] : 0u)) & KT_KEY_MALFORMED) != 0;
    if (malformed) { T.on_curve[id] = 0; return; }
    const kl_key k = kl_load_row(T, id);
    bool on = affine_on_curve(fq_from_words(k.u[0]), fq_from_words(k.v[0]));
    if (T.n_cols > 1) on = affine_on_curve(fq_from_words(k.u[1]), fq_from_words(k.v[1])) && on;
    T.on_curve[id] = on ? 1 : 0;
    uint32_t slot = (uint32_t)kl_hash_affine(T, k) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {      // at most half the slots are ever taken: ends long before
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t seen = atomicCAS(&T.slots[slot], KL_EMPTY, id);
#else
        const uint32_t seen = T.slots[slot];
        if (seen == KL_EMPTY) T.slots[slot] = id;
#endif
        if (seen == KL_EMPTY) return;
        // (whoever lowers this slot meanwhile has the bytes of `seen`: the comparison does not depend on which of them it reads)
        if (seen < T.n_keys && kl_same_affine(T, k, kl_load_row(T, seen))) {
#if defined(__HIP_DEVICE_COMPILE__)
            atomicMin(&T.slots[slot], id);
#else
            if (id < T.slots[slot]) T.slots[slot] = id;
#endif
            return;
        }
        slot = (slot + 1u) & T.mask;
    }
}

// The probe of an affine query (the canonical affine bytes of a key; anything else misses): the index, or KL_MISS.
JJS_HD uint32_t kl_find_affine(const keyset_lookup& T, const kl_key& q) {
    uint32_t slot = (uint32_t)kl_hash_affine(T, q) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const uint32_t c = T.slots[slot];
        if (c == KL_EMPTY) return KL_MISS;
        if (c < T.n_keys && kl_same_affine(T, q, kl_load_row(T, c))) return c;
        slot = (slot + 1u) & T.mask;
    }
    return KL_MISS;
}
// The probe of a wire query: e0 (e1) the 32-byte encodings of its point(s).
JJS_HD uint32_t kl_find_wire(const keyset_lookup& T, const words8& e0, const words8& e1) {
    uint32_t slot = (uint32_t)kl_hash(e0, e1, T.n_cols, T.seed) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const uint32_t c = T.slots[slot];
        if (c == KL_EMPTY) return KL_MISS;
        if (c < T.n_keys) {
            const kl_key r = kl_load_row(T, c);
            uint32_t d = kl_diff(e0, kl_encoding(r.u[0], r.v[0]));
            if (T.n_cols > 1) d |= kl_diff(e1, kl_encoding(r.u[1], r.v[1]));
            if (d == 0 && T.on_curve[c]) return c;
        }
        slot = (slot + 1u) & T.mask;
    }
    return KL_MISS;
}

// One item of a by-key call: its key column(s) K0 (K1) in `wire` or affine form -> the index of its key, or KL_MISS.  Wire:
// K0 holds n x 32 (one point column) or n x 64 (pk || pk'); affine: K0, K1 hold n x 64 each.
JJS_HD uint32_t kl_find_item(const keyset_lookup& T, bool wire, const uint8_t* K0, const uint8_t* K1, uint64_t item) {
    if (wire) {
        const fe_src s{K0, 32 * T.n_cols, 0};
        const words8 e0 = load_words(s, item);
        return kl_find_wire(T, e0, T.n_cols > 1 ? load_words(s, item, 32) : e0);
    }
    kl_key q{};
    const fe_src s0{K0, 64, 0};
    q.u[0] = load_words(s0, item); q.v[0] = load_words(s0, item, 32);
    if (T.n_cols > 1) {
        const fe_src s1{K1, 64, 0};
        q.u[1] = load_words(s1, item); q.v[1] = load_words(s1, item, 32);
    }
    return kl_find_affine(T, q);
}

// What a by-key call leaves of an item whose key is not in the set: the index pass ran it with a stand-in (ks_index_item: key 0,
// malformed), so no lane addressed the set for it; its status becomes KL_STATUS_NOT_IN_SET and leaves the tally.
constexpr uint32_t KL_STATUS_NOT_IN_SET = 6;
// true for a miss; *was = the status the stand-in run left behind (what the tally counted; without a status column that run's
// status is known: an index beyond the set is malformed)
JJS_HD bool kl_take_miss(const uint32_t* found, uint64_t item, uint8_t* status, uint32_t* was) {
    if (found[item] != KL_MISS) return false;
    *was = status ? (uint32_t)status[item] : (uint32_t)ST_MALFORMED;
    if (status) status[item] = (uint8_t)KL_STATUS_NOT_IN_SET;
    return true;
}

}  // namespace jjs

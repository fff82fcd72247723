// CPU build of csrc/keyset_add.h (adding keys to a live key set) for tests/test_keyset_add_host.py: the JJS_HD stage bodies the
// device runs -- probe, claim, mark, the scan of the block counts, gather, the answers -- in the order and the decomposition of
// the device's launches (blocks of BLOCK candidates, one scan block of KA_SCAN_LANES lanes), the flags of the new keys by the
// key-table path's own kt_key_flags, and the ranged insert into the set's lookup table beside a fresh build of the same set.
#include <map>
#include <string>

#include "keyset_lookup_harness.cpp"
#include "keyset_add.h"

namespace {

constexpr uint32_t KA_BLOCK = 256;       // BLOCK of device_kernels.h

struct aligned_rows {
    std::vector<uint8_t> mem;
    uint8_t* p = nullptr;
    void size(size_t rows) {
        mem.assign(rows * 64 + 80, 0);
        p = (uint8_t*)(((uintptr_t)mem.data() + 15) & ~(uintptr_t)15);
    }
};

// flags of keys [first, first + count) of a column from their rows, as key_chain_kernel's validity lane leaves them, with the
// malformed bit of keyset_flags_kernel
void key_flags(const uint8_t* rows, uint8_t* flags, const uint8_t* bad, uint32_t first, uint32_t count) {
    std::vector<uint32_t> ids(count);
    for (uint32_t i = 0; i < count; ++i) ids[i] = i;
    key_column C{};
    C.src = fe_src{rows + (size_t)first * 64, 64, 0};
    C.key_item = ids.data();
    C.key_flags = flags + first;
    static std::map<std::string, uint8_t> known;            // (the lists repeat their keys: one validity test per distinct point)
    for (uint32_t i = 0; i < count; ++i) {
        const std::string key((const char*)rows + ((size_t)first + i) * 64, 64);
        auto at = known.find(key);
        if (at == known.end()) {
            kt_key_flags(C, i);
            at = known.emplace(key, flags[first + i]).first;
        }
        flags[first + i] = at->second;
        if (bad && bad[i]) flags[first + i] |= (uint8_t)KT_KEY_MALFORMED;
    }
}

}  // namespace

extern "C" {

// The set: set0, set1 n_old x 64 affine rows as the set holds them, set_bad (nullable) the keys registered as malformed whatever
// their rows.  The candidates K0, K1 in `format` (0 affine, 1 ext, 2 wire: K0 alone, n x 32 x cols), `mode` 0 APPEND, 1 UNIQUE.
// Out: idx_out, status_out [n]; *n_added; rows_out [cols][n_old + n][64] and flags_out [cols][n_old + n] of the set afterwards
// (the first n_old + *n_added of each); slots_out: the lookup table after the add -- the new ids inserted into the old table, or
// every id into a table with more slots when the slot count grows (*rebuilt) -- and fresh_out: the table jjs_keyset_create
// would build over the same rows; both kl_slot_count(n_old + *n_added) slots.
int jjs_ka_host_add(uint32_t n_cols, int format, int mode, const uint8_t* set0, const uint8_t* set1, const uint8_t* set_bad, uint32_t n_old,
                    const uint8_t* K0, const uint8_t* K1, uint32_t n, uint64_t seed, uint32_t* idx_out, uint8_t* status_out, uint32_t* n_added,
                    uint8_t* rows_out, uint8_t* flags_out, uint32_t* slots_out, uint32_t* fresh_out, int* rebuilt) {
    if (n_cols < 1 || n_cols > 2 || n_old == 0 || n == 0 || format < 0 || format > 2 || mode < 0 || mode > 1) return -1;
    const uint32_t room = n_old + n;
    const uint8_t* set[2] = {set0, set1};
    aligned_rows rows[2], cand[2];
    std::vector<uint8_t> flags[2], bad(n, 0), on_curve(room, 0xAA);
    for (uint32_t c = 0; c < n_cols; ++c) {
        rows[c].size(room); cand[c].size(n);
        memcpy(rows[c].p, set[c], (size_t)n_old * 64);
        flags[c].assign(room, 0);
        key_flags(rows[c].p, flags[c].data(), set_bad, 0, n_old);
    }
    // the old set's lookup table
    std::vector<uint32_t> slots(kl_slot_count(n_old), KL_EMPTY);
    keyset_lookup S{};
    for (uint32_t c = 0; c < n_cols; ++c) { S.keys[c] = rows[c].p; S.flags[c] = flags[c].data(); }
    S.on_curve = on_curve.data(); S.slots = slots.data(); S.mask = (uint32_t)slots.size() - 1;
    S.n_keys = n_old; S.n_cols = n_cols; S.seed = seed;
    for (uint32_t i = 0; i < n_old; ++i) kl_insert(S, i);
    // the candidates' rows, as jjs_keyset_create's kernels make them
    if (format == 0) {
        const uint8_t* src[2] = {K0, K1};
        for (uint32_t c = 0; c < n_cols; ++c) memcpy(cand[c].p, src[c], (size_t)n * 64);
    } else if (format == 1) {
        std::vector<uint32_t> scratch(9 * (size_t)n + 16);
        normalize_params N{};
        N.n_src = n_cols; N.n = n; N.bad = bad.data(); N.scratch = scratch.data();
        const uint8_t* src[2] = {K0, K1};
        for (uint32_t c = 0; c < n_cols; ++c) { N.src[c] = fe_src{src[c], 96, 0}; N.out[c] = cand[c].p; }
        for (uint64_t lane = 0; lane < 64; ++lane) normalize_lane(N, lane, 64);
    } else {
        const dlog_tables T = host_dlog();
        std::map<std::string, decoded_point> decoded;           // (the lists repeat a few encodings: one square root each)
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t c = 0; c < n_cols; ++c) {
                words8 w;
                memcpy(w.w, K0 + ((size_t)i * n_cols + c) * 32, 32);
                const std::string key((const char*)w.w, 32);
                auto at = decoded.find(key);
                if (at == decoded.end()) at = decoded.emplace(key, decompress_point(w, T)).first;
                const decoded_point d = at->second;
                store_words(cand[c].p, 2 * (uint64_t)i, d.u);
                store_words(cand[c].p, 2 * (uint64_t)i + 1, d.v);
                if (!d.ok) bad[i] = 1;
            }
    }
    uint32_t n_add = n;
    std::vector<uint8_t> bad_new(n, 0);
    keyset_add_plan P{};
    const uint32_t blocks = (n + KA_BLOCK - 1) / KA_BLOCK;
    std::vector<uint8_t> skip(n), first(n), c_on_curve(n);
    std::vector<uint32_t> res(n), lead(n), rank(n), sums(blocks + 1), cslots(kl_slot_count(n), KL_EMPTY);
    if (mode == 1) {
        P.S = S;
        for (uint32_t c = 0; c < n_cols; ++c) { P.C.keys[c] = cand[c].p; P.C.flags[c] = skip.data(); P.dst[c] = rows[c].p + (size_t)n_old * 64; }
        P.C.on_curve = c_on_curve.data(); P.C.slots = cslots.data(); P.C.mask = (uint32_t)cslots.size() - 1;
        P.C.n_keys = n; P.C.n_cols = n_cols; P.C.seed = seed;
        P.bad = bad.data(); P.skip = skip.data(); P.res = res.data(); P.lead = lead.data(); P.first = first.data();
        P.sums = sums.data(); P.rank = rank.data(); P.n = n; P.n_old = n_old;
        for (uint32_t i = 0; i < n; ++i) ka_probe(P, i);
        for (uint32_t i = n; i-- > 0;) ka_claim(P, i);          // the lanes in the order least like the input's: the lowest position wins all the same
        for (uint32_t b = 0; b < blocks; ++b) {                 // keyset_add_mark_kernel: the block's count
            uint32_t count = 0;
            for (uint32_t i = b * KA_BLOCK; i < n && i < (b + 1) * KA_BLOCK; ++i) count += ka_mark(P, i);
            sums[b] = count;
        }
        {                                                       // keyset_add_scan_kernel
            uint32_t part[KA_SCAN_LANES], total = 0;
            for (uint32_t j = 0; j < KA_SCAN_LANES; ++j) part[j] = ka_scan_chunk_total(sums.data(), blocks, j);
            for (uint32_t j = 0; j < KA_SCAN_LANES; ++j) { ka_scan_chunk_write(sums.data(), blocks, j, total); total += part[j]; }
            sums[blocks] = total;
        }
        n_add = sums[blocks];
        for (uint32_t b = 0; b < blocks; ++b) {                 // keyset_add_gather_kernel: the rank inside the block
            uint32_t r = sums[b];
            for (uint32_t i = b * KA_BLOCK; i < n && i < (b + 1) * KA_BLOCK; ++i)
                if (first[i]) ka_gather(P, i, r++);
        }
    } else {
        for (uint32_t c = 0; c < n_cols; ++c) memcpy(rows[c].p + (size_t)n_old * 64, cand[c].p, (size_t)n * 64);
        bad_new = bad;
    }
    const uint32_t n_new = n_old + n_add;
    for (uint32_t c = 0; c < n_cols; ++c) key_flags(rows[c].p, flags[c].data(), bad_new.data(), n_old, n_add);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t idx = mode == 1 ? ka_index(P, i) : n_old + i;
        idx_out[i] = idx;
        status_out[i] = (uint8_t)ka_status(idx, n_cols, flags[0].data(), flags[1].data());
    }
    // the lookup table: the new ids in place, or every id into a table with more slots
    const uint32_t s_new = kl_slot_count(n_new);
    *rebuilt = s_new != (uint32_t)slots.size();
    keyset_lookup T = S;
    T.n_keys = n_new;
    std::vector<uint32_t> bigger;
    if (*rebuilt) {
        bigger.assign(s_new, KL_EMPTY);
        T.slots = bigger.data(); T.mask = s_new - 1;
        for (uint32_t i = 0; i < n_new; ++i) kl_insert(T, i);
    } else {
        for (uint32_t i = n_old; i < n_new; ++i) kl_insert(T, i);
    }
    memcpy(slots_out, T.slots, (size_t)s_new * 4);
    std::vector<uint32_t> fresh(s_new, KL_EMPTY);
    std::vector<uint8_t> fresh_on_curve(room, 0xAA);
    keyset_lookup F = T;
    F.slots = fresh.data(); F.on_curve = fresh_on_curve.data();
    for (uint32_t i = 0; i < n_new; ++i) kl_insert(F, i);
    memcpy(fresh_out, fresh.data(), (size_t)s_new * 4);
    if (memcmp(fresh_on_curve.data(), on_curve.data(), n_new)) return -2;      // the on-curve bytes of the grown set are those of a fresh one
    *n_added = n_add;
    for (uint32_t c = 0; c < n_cols; ++c) {
        memcpy(rows_out + (size_t)c * room * 64, rows[c].p, (size_t)n_new * 64);
        memcpy(flags_out + (size_t)c * room, flags[c].data(), n_new);
    }
    return 0;
}

// the scan alone, over `blocks` block counts (sums has blocks + 1 words): what keyset_add_scan_kernel leaves
void jjs_ka_host_scan(uint32_t* sums, uint32_t blocks) {
    uint32_t part[KA_SCAN_LANES], total = 0;
    for (uint32_t j = 0; j < KA_SCAN_LANES; ++j) part[j] = ka_scan_chunk_total(sums, blocks, j);
    for (uint32_t j = 0; j < KA_SCAN_LANES; ++j) { ka_scan_chunk_write(sums, blocks, j, total); total += part[j]; }
    sums[blocks] = total;
}

}  // extern "C"

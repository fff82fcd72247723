// CPU build of csrc/keyset_lookup.h (key sets by key) for tests/test_keyset_lookup_host.py: the JJS_HD insert and probe
// functions the device runs, with the seed, the slot count and the order of insertion as arguments, and the by-key
// verification of a batch: the probe, the index pass and the variants of keyset_harness.cpp, then the miss pass.
#include "keyset_harness.cpp"
#include "keyset_lookup.h"
#include "normalize.h"

namespace {

struct host_table {
    std::vector<uint8_t> flags[2], on_curve;
    std::vector<uint32_t> slots;
    keyset_lookup T{};
};

// keys0, keys1: n_keys x 64 (16-byte aligned); bad (nullable): keys the registration found malformed whatever their bytes (an
// encoding that did not decode); order (nullable): the order the keys are inserted in; slots 0: kl_slot_count(n_keys)
void build_table(host_table& H, uint32_t n_cols, const uint8_t* keys0, const uint8_t* keys1, const uint8_t* bad, uint32_t n_keys,
                 const uint32_t* order, uint64_t seed, uint32_t slots) {
    const uint8_t* keys[2] = {keys0, keys1};
    for (uint32_t c = 0; c < n_cols; ++c) {
        H.flags[c].assign(n_keys, 0);
        const fe_src s{keys[c], 64, 0};
        for (uint32_t k = 0; k < n_keys; ++k) {
            const bool canonical = words_lt(load_words(s, k), JJS_Q_WORDS) && words_lt(load_words(s, k, 32), JJS_Q_WORDS);
            H.flags[c][k] = (uint8_t)((canonical && !(bad && bad[k])) ? 0u : KT_KEY_MALFORMED);
        }
        H.T.keys[c] = keys[c];
        H.T.flags[c] = H.flags[c].data();
    }
    if (!slots) slots = kl_slot_count(n_keys);
    H.on_curve.assign(n_keys, 0xAA);
    H.slots.assign(slots, KL_EMPTY);
    H.T.on_curve = H.on_curve.data(); H.T.slots = H.slots.data(); H.T.mask = slots - 1;
    H.T.n_keys = n_keys; H.T.n_cols = n_cols; H.T.seed = seed;
    for (uint32_t i = 0; i < n_keys; ++i) kl_insert(H.T, order ? order[i] : i);
}

// the probe of n items in `format` (0 affine, 1 ext, 2 wire), extended keys normalised first as the device does (poison mode)
void find_items(const host_table& H, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint32_t* idx_out) {
    std::vector<uint8_t> norm[2];
    if (format == 1) {
        std::vector<uint32_t> scratch(9 * n + 9);
        normalize_params N{};
        N.n_src = H.T.n_cols; N.poison = 1; N.scratch = scratch.data(); N.n = n; N.first = 0;
        const uint8_t* src[2] = {K0, K1};
        for (uint32_t c = 0; c < H.T.n_cols; ++c) {
            norm[c].assign(64 * n + 80, 0);
            N.src[c] = fe_src{src[c], 96, 0};
            N.out[c] = (uint8_t*)(((uintptr_t)norm[c].data() + 15) & ~(uintptr_t)15);
        }
        normalize_lane<true>(N, 0, 1);
        K0 = N.out[0]; K1 = N.out[1];
    }
    for (size_t i = 0; i < n; ++i) idx_out[i] = kl_find_item(H.T, format == 2, K0, K1, i);
}

}  // namespace

extern "C" {

uint32_t jjs_kl_slot_count(uint32_t n_keys) { return kl_slot_count(n_keys); }

// the hash of one key (its points' 64-byte affine rows) under `seed`: what tests/keyset_lookup_cases.py restates
uint64_t jjs_kl_hash_affine(uint32_t n_cols, const uint8_t* p0, const uint8_t* p1, uint64_t seed) {
    keyset_lookup T{};
    T.keys[0] = p0; T.keys[1] = p1; T.n_cols = n_cols; T.seed = seed;
    return kl_hash_affine(T, kl_load_row(T, 0));
}

// slots_out (nullable): the table's slots; on_curve_out (nullable): the on-curve byte per key
int jjs_kl_host_find(uint32_t n_cols, const uint8_t* keys0, const uint8_t* keys1, const uint8_t* bad, uint32_t n_keys, const uint32_t* order,
                     uint64_t seed, uint32_t slots, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint32_t* idx_out,
                     uint32_t* slots_out, uint8_t* on_curve_out) {
    if (n_cols < 1 || n_cols > 2 || n_keys == 0 || format < 0 || format > 2 || (slots & (slots - 1))) return -1;
    host_table H;
    build_table(H, n_cols, keys0, keys1, bad, n_keys, order, seed, slots);
    find_items(H, format, K0, K1, n, idx_out);
    if (slots_out) memcpy(slots_out, H.slots.data(), H.slots.size() * 4);
    if (on_curve_out) memcpy(on_curve_out, H.on_curve.data(), n_keys);
    return 0;
}

// By-key verification of a batch of affine columns (the arguments of jjs_keyset_host_verify with the key columns K0, K1 in
// place of key_idx): a hit runs with the index the probe found, a miss with the stand-in of an index beyond the set, then the
// miss pass.  tally[4]: the statuses 0 .. 3 counted, the misses in none.
int jjs_kl_host_verify_keys(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys, uint64_t seed, const uint8_t* K0,
                            const uint8_t* K1, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m, size_t n, int positions,
                            uint8_t* status, uint64_t* tally, uint32_t* idx_out) {
    host_table H;
    build_table(H, scheme == 0 ? 1u : 2u, keys0, keys1, nullptr, n_keys, nullptr, seed, 0);
    find_items(H, 0, K0, K1, n, idx_out);
    std::vector<uint8_t> key_status(n_keys);
    if (int rc = jjs_keyset_host_verify(scheme, keys0, keys1, n_keys, idx_out, u, R, Rp, m, n, positions, status, key_status.data())) return rc;
    for (int k = 0; k < 4; ++k) tally[k] = 0;
    for (size_t i = 0; i < n; ++i) ++tally[status[i] & 3];
    for (size_t i = 0; i < n; ++i) {
        uint32_t was = 0;
        if (kl_take_miss(idx_out, i, status, &was)) --tally[was & 3];
    }
    return 0;
}

}  // extern "C"

// CPU build of csrc/keyset.h (registered key sets) for tests/test_keyset_host.py: a set is built with the key-table path's
// own per-key functions (kt_chain_key, kt_table_lane), a call runs the index pass, the keyed hash and either variant --
// kt_finish_item (one lane per item) or ks_small_item_serial (the latency variant's lanes in turn) -- then the resolve pass.
// The comb tables, the double scheme's tag and the other CPU entry points come from host_harness.cpp.
#include "host_harness.cpp"
#include "keyset.h"

extern "C" {

// scheme 0 / 1 / 2; keys0, keys1: n_keys x 64 affine (keys1 NULL for single); positions 0 = the large variant, else 4, 8, 16
int jjs_keyset_host_verify(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys, const uint32_t* key_idx,
                           const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m, size_t n, int positions,
                           uint8_t* status, uint8_t* key_status) {
    if (scheme < 0 || scheme > 2 || n_keys == 0 || (positions && positions != 4 && positions != 8 && positions != 16)) return -1;
    ensure_tables();
    const int w = KEYSET_WINDOW;
    const uint32_t cols = scheme == 0 ? 1u : 2u;
    const uint8_t* keys[2] = {keys0, keys1};
    std::vector<uint32_t> key_item(n_keys), tables[2], bases[2], keyid(n + 1);
    std::vector<uint8_t> flags[2], gathered[2], bad(n + 1, 0);
    for (uint32_t k = 0; k < n_keys; ++k) key_item[k] = k;
    key_params K{};
    K.n_cols = cols; K.max_keys = n_keys; K.n = n;
    for (uint32_t c = 0; c < cols; ++c) {
        key_column& C = K.col[c];
        flags[c].assign(n_keys, 0);
        bases[c].assign((size_t)n_keys * kt_positions(w) * KT_BASE_WORDS + 4, 0);
        tables[c].assign((size_t)n_keys * kt_positions(w) * kt_table_words(w) + 8, 0);
        gathered[c].assign(64 * n + 64, 0);
        C.src = fe_src{keys[c], 64, 0};
        C.key_item = key_item.data(); C.key_flags = flags[c].data(); C.bases = bases[c].data();
        C.tables = (uint32_t*)(((uintptr_t)tables[c].data() + 15) & ~(uintptr_t)15);
        C.keyid = keyid.data();
        for (uint32_t k = 0; k < n_keys; ++k) {
            if (!kt_chain_key(C, k, w)) continue;             // tables for the valid keys only, as on the device
            for (uint32_t pos = 0; pos < (uint32_t)kt_positions(w); ++pos) kt_table_lane(C, k, pos, w);
        }
    }
    if (key_status)
        for (uint32_t k = 0; k < n_keys; ++k) key_status[k] = (uint8_t)ks_key_status(flags[0][k], cols > 1 ? flags[1][k] : (uint32_t)KT_KEY_VALID);
    uint8_t* g0 = (uint8_t*)(((uintptr_t)gathered[0].data() + 15) & ~(uintptr_t)15);
    uint8_t* g1 = cols > 1 ? (uint8_t*)(((uintptr_t)gathered[1].data() + 15) & ~(uintptr_t)15) : nullptr;
    for (uint64_t i = 0; i < n; ++i) ks_index_item(key_idx, n_keys, i, keyid.data(), bad.data(), cols, keys0, keys1, g0, g1);
    const out_ptrs o{status, nullptr, nullptr, nullptr};
    verify_params P = scheme == 0 ? params_single(u, R, g0, m, n, g_comb_g.data(), o)
                    : scheme == 1 ? params_double(u, R, Rp, g0, g1, m, n, (const uint8_t*)g_tag, g_comb_g.data(), g_comb_gn.data(), o)
                                  : params_vargen(u, R, g0, g1, m, n, o);
    uint32_t window = (uint32_t)w;
    P.key_flag = &window;
    P.pre_malformed = bad.data();
    for (uint64_t i = 0; i < n; ++i) {
        const prep_record r = prepare_item(P, i);
        uint32_t st = positions ? ks_small_item_serial(P, K, i, (uint32_t)positions, r) : kt_finish_item(P, K, i, r);
        if (st >= ST_PENDING_EQ_FAILED) st = resolve_item(P, i, st == ST_PENDING_EQ_HELD);
        status[i] = (uint8_t)st;
    }
    return 0;
}

}  // extern "C"

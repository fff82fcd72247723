// CPU build of csrc/keyset_verdict.h (the batch verdict against a registered key set, jjs_keyset_verify_all*) for
// tests/test_keyset_verify_all_host.py and tests/test_msm_host.py: the device's steps run here in loops with the same functions -- the set built as
// keyset_harness.cpp builds it, the index pass, the keyed item pass (ksv_item), the counting sort by key, the heads and
// cells of the runs, the key points (ksv_key_point), the bucket method (host_msm.h) over the R terms with the short
// weights' windows, bv_verdict.  The comb tables and the double scheme's tag come from host_harness.cpp.
#include "host_harness.cpp"
#include "keyset_verdict.h"
#include "host_msm.h"

namespace {

// a set built as keyset_harness.cpp builds it: flags, bases and window tables per point column (tables for the valid keys
// only, as on the device; with poison the tables of the others are filled with 0xFF), the items' clamped key indices
struct host_set {
    uint32_t cols, n_keys;
    std::vector<uint32_t> key_item, tables[2], bases[2], keyid;
    std::vector<uint8_t> flags[2];
    key_column col[2] = {};

    host_set(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys_, size_t n, int poison)
        : cols(scheme == 0 ? 1u : 2u), n_keys(n_keys_), key_item(n_keys_), keyid(n + 1) {
        const int w = KEYSET_WINDOW;
        const uint8_t* keys[2] = {keys0, keys1};
        for (uint32_t k = 0; k < n_keys; ++k) key_item[k] = k;
        const size_t key_table_words = (size_t)kt_positions(w) * kt_table_words(w);
        for (uint32_t ci = 0; ci < cols; ++ci) {
            key_column& C = col[ci];
            flags[ci].assign(n_keys, 0);
            bases[ci].assign((size_t)n_keys * kt_positions(w) * KT_BASE_WORDS + 4, 0);
            tables[ci].assign((size_t)n_keys * key_table_words + 8, 0);
            C.src = fe_src{keys[ci], 64, 0};
            C.key_item = key_item.data(); C.key_flags = flags[ci].data(); C.bases = bases[ci].data();
            C.tables = align16(tables[ci]);
            C.keyid = keyid.data();
            for (uint32_t k = 0; k < n_keys; ++k) {
                if (kt_chain_key(C, k, w)) {
                    for (uint32_t pos = 0; pos < (uint32_t)kt_positions(w); ++pos) kt_table_lane(C, k, pos, w);
                } else if (poison) {
                    memset(C.tables + (size_t)k * key_table_words, 0xFF, key_table_words * 4);
                }
            }
        }
    }
};

// the counting sort by key: counts, exclusive scan, scatter (the cursors end at the ends of the runs)
void sort_by_key(const std::vector<uint32_t>& keyid, uint32_t n_keys, size_t n, std::vector<uint32_t>& cursor, std::vector<uint32_t>& order) {
    cursor.assign(n_keys, 0); order.assign(n, 0);
    for (uint64_t i = 0; i < n; ++i) ++cursor[keyid[i]];
    uint32_t run = 0;
    for (uint32_t k = 0; k < n_keys; ++k) { const uint32_t cnt = cursor[k]; cursor[k] = run; run += cnt; }
    for (uint64_t i = 0; i < n; ++i) order[cursor[keyid[i]]++] = (uint32_t)i;
}

}  // namespace

extern "C" {

// The run sums and the key points alone, under the caller's own scalar columns, for n_cases cases against one set: case i has
// ns[i] items, its key indices and its columns a0, a1 (32 bytes per item, below r; a1 NULL for single) follow those of case
// i - 1.  sums_out = per case the S_k of point column 0 then 1 (n_keys x 32 each), point_out = per case the affine sum of
// S_k * P_k (64 bytes).
int jjs_ksv_host_key_sums(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys, size_t n_cases, const size_t* ns,
                          const uint32_t* key_idx, const uint8_t* a0, const uint8_t* a1, int poison, uint8_t* sums_out, uint8_t* point_out) {
    if (scheme < 0 || scheme > 2 || n_keys == 0 || !ns || !sums_out || !point_out) return -1;
    size_t n_max = 0;
    for (size_t i = 0; i < n_cases; ++i) n_max = ns[i] > n_max ? ns[i] : n_max;
    host_set set(scheme, keys0, keys1, n_keys, n_max, poison);
    size_t first = 0;
    for (size_t ci = 0; ci < n_cases; first += ns[ci], ++ci) {
        const size_t n = ns[ci];
        if (n == 0) return -1;
        for (uint64_t i = 0; i < n; ++i) {
            if (key_idx[first + i] >= n_keys) return -1;
            set.keyid[i] = key_idx[first + i];
        }
        std::vector<uint32_t> cursor, order;
        sort_by_key(set.keyid, n_keys, n, cursor, order);
        const ksv_runs Rn{cursor.data(), 1u, order.data(), set.keyid.data(), n_keys, n};
        const uint32_t cells = ksv_cells(n);
        const uint8_t* a[2] = {a0 + 32 * first, a1 ? a1 + 32 * first : nullptr};
        uint8_t* sums = sums_out + ci * set.cols * n_keys * 32;
        ext_pt total = ext_identity();
        for (uint32_t col = 0; col < set.cols; ++col) {
            std::vector<uint8_t> head((size_t)n_keys * 32 + 16), cell((size_t)cells * 32 + 16);
            uint8_t *h = align16(head), *cl = align16(cell);
            for (uint32_t k = 0; k < n_keys; ++k) store_words(h, k, ksv_head(Rn, a[col], k));
            for (uint32_t g = 0; g < cells; ++g) store_words(cl, g, ksv_cell(Rn, a[col], g));
            for (uint32_t k = 0; k < n_keys; ++k) {
                total = msm_add_ext(total, ksv_key_point(Rn, set.col[col], h, cl, k));
                store_words(sums, (uint64_t)col * n_keys + k, ksv_key_sum(Rn, h, cl, k));
            }
        }
        to_affine_bytes(total, point_out + 64 * ci);
    }
    return 0;
}

// scheme 0 / 1 / 2; keys0, keys1: n_keys x 64 affine (keys1 NULL for single); affine signature columns; seed: 32 bytes;
// c: the window width of the bucket method (0: by size); poison: the tables of the keys that are not valid are filled with
// 0xFF before the call.  Outputs (nullable): total = the affine sum (sum z u) G + sum_k S_k PK_k - sum z_i R_i (64 bytes),
// key_sums = the S_k of point column 0 then 1 (n_keys x 32 each), key_status, z_bits = the bits of the weights.
// The item pass alone (items != 0), as jjs_debug_keyset_items_dev copies it out on the device: scalars_out = the n_eq * n
// weights, a_out[0], a_out[1] = the items' scalars on their key's point columns (n x 32), partial_out = for each grid of
// grids[0 .. n_grids) the partial sums of its blocks (item i belongs to block (i / 256) mod blocks; 64 bytes per block, grid after
// grid), fail_out, zu_out = the two totals (64 bytes).
static int ksv_host_run(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys, const uint32_t* key_idx,
                        const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m, size_t n, const uint8_t seed[32],
                        int c, int poison, int* verdict, uint8_t* total_out, uint8_t* key_sums, uint8_t* key_status, int* z_bits,
                        int items, const uint32_t* grids, size_t n_grids, uint8_t* scalars_out, uint8_t* const* a_out, uint8_t* partial_out, uint32_t* fail_out,
                        uint8_t* zu_out) {
    if (scheme < 0 || scheme > 2 || n_keys == 0 || n == 0) return -1;
    ensure_tables();
    const int w = KEYSET_WINDOW;
    host_set set(scheme, keys0, keys1, n_keys, n, poison);
    const uint32_t cols = set.cols;
    std::vector<uint32_t>& keyid = set.keyid;
    std::vector<uint8_t>* flags = set.flags;
    key_column* col = set.col;
    std::vector<uint8_t> gathered[2], bad(n + 1, 0);
    for (uint32_t ci = 0; ci < cols; ++ci) gathered[ci].assign(64 * n + 64, 0);
    if (key_status)
        for (uint32_t k = 0; k < n_keys; ++k) key_status[k] = (uint8_t)ks_key_status(flags[0][k], cols > 1 ? flags[1][k] : (uint32_t)KT_KEY_VALID);
    uint8_t* g0 = align16(gathered[0]);
    uint8_t* g1 = cols > 1 ? align16(gathered[1]) : nullptr;
    for (uint64_t i = 0; i < n; ++i) ks_index_item(key_idx, n_keys, i, keyid.data(), bad.data(), cols, keys0, keys1, g0, g1);
    const out_ptrs o{nullptr, nullptr, nullptr, nullptr};
    ksv_params B{};
    B.V = scheme == 0 ? params_single(u, R, g0, m, n, g_comb_g.data(), o)
        : scheme == 1 ? params_double(u, R, Rp, g0, g1, m, n, (const uint8_t*)g_tag, g_comb_g.data(), g_comb_gn.data(), o)
                      : params_vargen(u, R, g0, g1, m, n, o);
    uint32_t window = (uint32_t)w;
    B.V.key_flag = &window;
    B.V.pre_malformed = bad.data();
    memcpy(B.seed, seed, 32);
    B.n_cols = cols; B.keyid = keyid.data();
    B.key_flags[0] = flags[0].data(); B.key_flags[1] = cols > 1 ? flags[1].data() : nullptr;
    const size_t N = (size_t)B.V.n_eq * n;
    if (c == 0) c = msm_pick_short_window(N);
    if (c < 8 || c > MSM_MAX_WINDOW) return -1;
    B.z_bits = msm_weight_bits(c);
    if (z_bits) *z_bits = B.z_bits;
    std::vector<uint32_t> terms(N * MSM_TERM_WORDS + 4);
    std::vector<uint8_t> scalars(N * 32 + 16), a[2], head[2], cell[2];
    B.terms = align16(terms); B.scalars = align16(scalars);
    const uint32_t cells = ksv_cells(n);
    for (uint32_t ci = 0; ci < 2; ++ci) {
        a[ci].assign(n * 32 + 16, 0); head[ci].assign((size_t)n_keys * 32 + 16, 0); cell[ci].assign((size_t)cells * 32 + 16, 0);
        B.a[ci] = align16(a[ci]);
    }
    bool failed = false;
    words8 sum[2] = {words_zero(), words_zero()};
    std::vector<words8> per_item;
    for (uint64_t i = 0; i < n; ++i) {
        words8 zu[2];
        failed = !ksv_item(B, i, zu) || failed;
        for (int e = 0; e < 2; ++e) {
            sum[e] = fr_add(sum[e], zu[e]);
            per_item.push_back(zu[e]);
        }
    }
    if (items) {
        memcpy(scalars_out, B.scalars, N * 32);
        for (uint32_t ci = 0; ci < cols; ++ci) memcpy(a_out[ci], B.a[ci], n * 32);
        for (size_t g = 0; g < n_grids; ++g) {
            if (grids[g] == 0) return -1;
            std::vector<words8> part(2 * (size_t)grids[g], words_zero());
            for (uint64_t i = 0; i < n; ++i)
                for (int e = 0; e < 2; ++e) {
                    words8& p = part[2 * (size_t)((i / 256) % grids[g]) + e];
                    p = fr_add(p, per_item[2 * i + e]);
                }
            memcpy(partial_out, part.data(), 64 * (size_t)grids[g]);
            partial_out += 64 * (size_t)grids[g];
        }
        *fail_out = failed ? 1u : 0u;
        memcpy(zu_out, sum[0].w, 32); memcpy(zu_out + 32, sum[1].w, 32);
        return 0;
    }
    std::vector<uint32_t> cursor, order;
    sort_by_key(keyid, n_keys, n, cursor, order);
    const ksv_runs Rn{cursor.data(), 1u, order.data(), keyid.data(), n_keys, n};
    ext_pt total = host_msm(B.terms, B.scalars, N, msm_shape_short(c), [](uint64_t) { return true; });     // every term is a -R
    for (uint32_t ci = 0; ci < cols; ++ci) {
        uint8_t *h = align16(head[ci]), *cl = align16(cell[ci]);
        for (uint32_t k = 0; k < n_keys; ++k) store_words(h, k, ksv_head(Rn, B.a[ci], k));
        for (uint32_t g = 0; g < cells; ++g) store_words(cl, g, ksv_cell(Rn, B.a[ci], g));
        for (uint32_t k = 0; k < n_keys; ++k) {
            total = msm_add_ext(total, ksv_key_point(Rn, col[ci], h, cl, k));
            if (key_sums) store_words(key_sums, (uint64_t)ci * n_keys + k, ksv_key_sum(Rn, h, cl, k));
        }
    }
    *verdict = bv_verdict(B.V, total, sum, failed) ? 1 : 0;
    if (total_out) {
        for (uint32_t e = 0; e < B.V.n_eq; ++e)
            if (B.V.eq[e].comb) total = add_comb_range(total, B.V.eq[e].comb, sum[e], 0, COMB_WINDOWS, true);
        to_affine_bytes(total, total_out);
    }
    return 0;
}
int jjs_ksv_host_verify_all(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys, const uint32_t* key_idx,
                            const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m, size_t n, const uint8_t seed[32],
                            int c, int poison, int* verdict, uint8_t* total_out, uint8_t* key_sums, uint8_t* key_status, int* z_bits) {
    if (!verdict) return -1;
    return ksv_host_run(scheme, keys0, keys1, n_keys, key_idx, u, R, Rp, m, n, seed, c, poison, verdict, total_out, key_sums, key_status, z_bits,
                        0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int jjs_ksv_host_items(int scheme, const uint8_t* keys0, const uint8_t* keys1, uint32_t n_keys, const uint32_t* key_idx, const uint8_t* u,
                       const uint8_t* R, const uint8_t* Rp, const uint8_t* m, size_t n, const uint8_t seed[32], int c, const uint32_t* grids,
                       size_t n_grids, uint8_t* scalars_out, uint8_t* a0_out, uint8_t* a1_out, uint8_t* partial_out, uint32_t* fail_out, uint8_t* zu_out) {
    if (c < 8 || !scalars_out || !a0_out || !partial_out || !fail_out || !zu_out) return -1;
    uint8_t* const a_out[2] = {a0_out, a1_out};
    return ksv_host_run(scheme, keys0, keys1, n_keys, key_idx, u, R, Rp, m, n, seed, c, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                        1, grids, n_grids, scalars_out, a_out, partial_out, fail_out, zu_out);
}

}  // extern "C"

// CPU build of csrc/batch_verdict.h and csrc/msm.h (the batch verdict of jjs_verify_all_*) for tests/test_verify_all_host.py and
// tests/test_msm_host.py:
// the device's steps run here in loops -- the per-item pass (bv_item), then the bucket method (host_msm.h) -- with the same
// functions.  The comb tables and the double scheme's tag come from host_harness.cpp.
#include "host_harness.cpp"
#include "batch_verdict.h"
#include "host_msm.h"

namespace {

// the item pass of verdict_item_pass on this thread: every item through item_fn in turn, its z u (z' u) kept per item and
// added to the total
template <class P, class Item>
bool host_item_pass(const P& B, uint64_t n, Item item_fn, words8 sum[2], std::vector<words8>* per_item) {
    bool failed = false;
    sum[0] = words_zero(); sum[1] = words_zero();
    for (uint64_t i = 0; i < n; ++i) {
        words8 zu[2];
        failed = !item_fn(B, i, zu) || failed;
        for (int e = 0; e < 2; ++e) {
            sum[e] = fr_add(sum[e], zu[e]);
            if (per_item) per_item->push_back(zu[e]);
        }
    }
    return failed;
}
// ... and the partial sums the device's blocks leave for each grid of grids[0 .. n_grids): item i belongs to block
// (i / 256) mod blocks (the grid-stride loop of `blocks` blocks of 256 lanes); 64 bytes per block, grid after grid
inline void host_block_sums(const std::vector<words8>& per_item, uint64_t n, const uint32_t* grids, size_t n_grids, uint8_t* partial_out) {
    for (size_t g = 0; g < n_grids; ++g) {
        std::vector<words8> part(2 * (size_t)grids[g], words_zero());
        for (uint64_t i = 0; i < n; ++i) {
            const size_t b = (size_t)((i / 256) % grids[g]);
            for (int e = 0; e < 2; ++e) part[2 * b + e] = fr_add(part[2 * b + e], per_item[2 * i + e]);
        }
        memcpy(partial_out, part.data(), 64 * (size_t)grids[g]);
        partial_out += 64 * (size_t)grids[g];
    }
}

// the descriptor of a verdict call over the scheme's columns, its terms and scalars in the vectors
struct host_verdict {
    bv_params B{};
    size_t N = 0;
    std::vector<uint32_t> terms;
    std::vector<uint8_t> scalars;
    host_verdict(int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PK2, const uint8_t* m,
                 size_t n, const uint8_t seed[32]) {
        const out_ptrs o{nullptr, nullptr, nullptr, nullptr};
        B.V = scheme == 0 ? params_single(u, R, PK, m, n, g_comb_g.data(), o)
            : scheme == 1 ? params_double(u, R, Rp, PK, PK2, m, n, (const uint8_t*)g_tag, g_comb_g.data(), g_comb_gn.data(), o)
                          : params_vargen(u, R, PK, PK2, m, n, o);
        memcpy(B.seed, seed, 32);
        B.n_kinds = bv_kinds(B.V);
        N = (size_t)B.n_kinds * n;
        terms.resize(N * MSM_TERM_WORDS + 4);
        scalars.resize(N * 32 + 16);
        B.terms = align16(terms); B.scalars = align16(scalars);
    }
};

}  // namespace

extern "C" {

int jjs_vh_chacha20_block(const uint8_t key[32], uint32_t counter, const uint8_t nonce[12], uint8_t out[64]) {
    uint32_t k[8], nn[3], o[16];
    memcpy(k, key, 32);
    memcpy(nn, nonce, 12);
    chacha20_block(k, counter, nn, o);
    memcpy(out, o, 64);
    return 0;
}

// points: N x 64 affine (u || v, canonical little-endian); scalars: N x 32 (< 2^252; short_shape != 0: within
// msm_weight_bits(c) bits, the windows of msm_shape_short); neg: N flags; c: window width (0: by N).
// out: the affine sum (64 bytes).  Nullable: off_out (W * B + 1 words), order_out (room for N * W words; off[W * B] are
// written), win_out (W affine window sums of 64 bytes)
int jjs_vh_msm(const uint8_t* points, const uint8_t* scalars, const uint8_t* neg, size_t N, int c, int short_shape, uint8_t* out,
               uint32_t* off_out, uint32_t* order_out, uint8_t* win_out) {
    if (c == 0) c = short_shape ? msm_pick_short_window(N) : msm_pick_window(N);
    if (c < 2 || c > MSM_MAX_WINDOW) return -1;
    std::vector<uint32_t> terms(N * MSM_TERM_WORDS + 4);
    uint32_t* t = align16(terms);
    const fe_src src{points, 64, 0};
    for (size_t i = 0; i < N; ++i) msm_store_term(t + i * MSM_TERM_WORDS, load_fq(src, i), load_fq(src, i, 32));
    const msm_shape S = short_shape ? msm_shape_short(c) : msm_shape_full(c);
    host_msm_stages st;
    to_affine_bytes(host_msm(t, scalars, N, S, [&](uint64_t i) { return neg[i] != 0; }, &st), out);
    if (off_out) memcpy(off_out, st.off.data(), st.off.size() * 4);
    if (order_out) memcpy(order_out, st.order.data(), st.order.size() * 4);
    if (win_out)
        for (int j = 0; j < S.W; ++j) to_affine_bytes(msm_load_ext(&st.win[(size_t)j * MSM_EXT_WORDS]), win_out + 64 * j);
    return 0;
}

// scheme 0 / 1 / 2, columns in the order of jjs_verify_*; p4 = PK' (double) or unused; seed: 32 bytes; c: window (0: by size)
int jjs_vh_verify_all(int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PK2,
                      const uint8_t* m, size_t n, const uint8_t seed[32], int c, int* verdict) {
    if (scheme < 0 || scheme > 2 || !verdict) return -1;
    if (n == 0) { *verdict = 1; return 0; }
    ensure_tables();
    host_verdict H(scheme, u, R, Rp, PK, PK2, m, n, seed);
    bv_params& B = H.B;
    if (c == 0) c = msm_pick_window(H.N);
    B.z_bits = msm_weight_bits(c);
    words8 sum[2];
    const bool failed = host_item_pass(B, n, [](const bv_params& b, uint64_t i, words8* zu) { return bv_item(b, i, zu); }, sum, nullptr);
    const ext_pt total = host_msm(B.terms, B.scalars, H.N, msm_shape_full(c), [&](uint64_t t) { return bv_kind_negated(B.V, (uint32_t)(t / n)); });
    *verdict = bv_verdict(B.V, total, sum, failed) ? 1 : 0;
    return 0;
}

// The item pass alone, as jjs_debug_verdict_items_dev copies it out on the device: the n_kinds * n scalars, the fail word, the
// two totals (64 bytes) and, for each of the n_grids grids, the partial sums of its blocks (64 bytes each, grid after grid).
// c: the window width that gives the weights' bits.
int jjs_vh_verdict_items(int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PK2,
                         const uint8_t* m, size_t n, const uint8_t seed[32], int c, const uint32_t* grids, size_t n_grids, uint8_t* scalars_out,
                         uint8_t* partial_out, uint32_t* fail_out, uint8_t* zu_out) {
    if (scheme < 0 || scheme > 2 || n == 0 || c < 8 || c > MSM_MAX_WINDOW) return -1;
    for (size_t g = 0; g < n_grids; ++g)
        if (grids[g] == 0) return -1;
    ensure_tables();
    host_verdict H(scheme, u, R, Rp, PK, PK2, m, n, seed);
    H.B.z_bits = msm_weight_bits(c);
    words8 sum[2];
    std::vector<words8> per_item;
    const bool failed = host_item_pass(H.B, n, [](const bv_params& b, uint64_t i, words8* zu) { return bv_item(b, i, zu); }, sum, &per_item);
    host_block_sums(per_item, n, grids, n_grids, partial_out);
    memcpy(scalars_out, H.B.scalars, H.N * 32);
    *fail_out = failed ? 1u : 0u;
    memcpy(zu_out, sum[0].w, 32); memcpy(zu_out + 32, sum[1].w, 32);
    return 0;
}

}  // extern "C"

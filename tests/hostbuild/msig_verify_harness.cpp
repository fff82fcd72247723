// CPU build of csrc/msig_verify.h (the verifier's half of the multisignature scheme) for tests/test_msig_verify_host.py: the
// passes one item after the other in the order the device launches them -- normalize_lane in poison mode for an extended call,
// the map, the check (or, for a key set registered here with the kt_* builders as in msig_keyset_harness.cpp, the gather),
// the delinearisation, the sum -- then, for a verification call, the CPU build's single-scheme verification on the aggregate
// column (host_harness.cpp `run`) and the clear pass.  The comb table and ext_normalize come from host_harness.cpp and
// msig_ext_harness.cpp.
#include "msig_ext_harness.cpp"
#include "msig_verify.h"

extern "C" {

// keys: n_keys x 64 affine, the set of a key-set call (NULL: an inline call).  rows: N x 64 / N x 96 keys, or N x uint32
// indices.  ext: the format of the inline keys and of R.  u NULL: aggregation alone (vec_status out), else verification
// (status, tally out).  lanes: the launch shape of the normalisation.  Every pointer is 16-byte aligned.
int jjs_msig_verify_host(const uint8_t* keys, size_t n_keys, const void* rows, int ext, const uint32_t* offsets, size_t B, size_t lanes,
                         const uint8_t* u, const uint8_t* R, const uint8_t* m, uint8_t* agg_pk, uint8_t* vec_status, uint8_t* status,
                         uint64_t* tally) {
    ensure_tables();
    auto aligned = [](std::vector<uint32_t>& v) { return (uint32_t*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); };
    const bool keyset = keys != nullptr, verify = u != nullptr;
    const size_t n = offsets[B];
    const int w = KEYSET_WINDOW;
    // ---- registration (a key-set call) ----
    std::vector<uint32_t> key_item(n_keys + 1), bases, tables, key_bytes(n_keys * 16 + 4);
    std::vector<uint8_t> flags(n_keys + 1, 0);
    key_column C{};
    uint8_t* kb = (uint8_t*)aligned(key_bytes);
    if (keyset) {
        if (n_keys == 0 || n_keys > KEYSET_MAX_KEYS) return -1;
        bases.resize(n_keys * (size_t)kt_positions(w) * KT_BASE_WORDS + 4);
        tables.assign(n_keys * (size_t)kt_positions(w) * kt_table_words(w) + 4, 0u);
        memcpy(kb, keys, n_keys * 64);
        C.src = fe_src{kb, 64, 0};
        C.key_item = key_item.data(); C.key_flags = flags.data(); C.bases = aligned(bases); C.tables = aligned(tables);
        for (uint32_t id = 0; id < n_keys; ++id) {
            key_item[id] = id;
            if (kt_chain_key(C, id, w))
                for (uint32_t pos = 0; pos < (uint32_t)kt_positions(w); ++pos) kt_table_lane(C, id, pos, w);
        }
    }
    // ---- the call ----
    column pk_norm(n + 1), r_norm(B + 1), gathered(n + 1), agg(B + 1);
    const uint8_t *pk = keyset ? nullptr : (const uint8_t*)rows, *r = R;
    if (ext && !keyset && n) {
        uint8_t* out[1] = {pk_norm.p()};
        ext_normalize(&pk, 1, n, lanes, 1, out, nullptr);
        pk = pk_norm.p();
    }
    if (ext && verify) {
        uint8_t* out[1] = {r_norm.p()};
        ext_normalize(&r, 1, B, lanes, 1, out, nullptr);
        r = r_norm.p();
    }
    std::vector<uint32_t> tr(n + 1), d(8 * n + 8), dpk(EXT_WORDS * n + 4), ws(WS_WORDS_PER_LANE + 4), long_tags(18 * B + 18, 0u), row_key(n + 1),
        refused(B + 1, 0u);
    msig_verify_keyset_params VK{};
    msig_params& P = VK.K.M;
    P.offsets = offsets; P.n_transcripts = (uint32_t)B; P.n_total = n;
    P.agg_pk = agg.p();
    P.tr_of = tr.data(); P.d_words = d.data(); P.dpk = dpk.data();
    P.tags = &JJS_SPONGE_TAG_LONG[0][0]; P.comb_g = g_comb_g.data();
    P.max_table_participants = JJS_MSIG_MAX_PARTICIPANTS;
    P.long_tags = long_tags.data();
    VK.K.refused = refused.data();
    VK.vec_status = vec_status; VK.poison = verify ? 1u : 0u;
    if (keyset) {
        msig_keyset_params& K = VK.K;
        K.key_idx = (const uint32_t*)rows; K.n_keys = (uint32_t)n_keys;
        K.keys = kb; K.flags = flags.data(); K.tables = C.tables;
        K.pk_col = gathered.p(); K.row_key = row_key.data();
        P.PK = K.pk_col;
    } else {
        P.PK = pk;
    }
    uint32_t* lane_ws = aligned(ws);
    for (size_t t = 0; t < B; ++t) msig_map_item(P, (uint32_t)t);
    const msig_verify_params V = mv_of(VK);
    for (size_t i = 0; i < n; ++i) {
        if (keyset) mk_gather_item(VK.K, i);
        else mv_check_item(V, i);
    }
    for (size_t i = 0; i < n; ++i) {
        if (keyset) mk_delin_item(VK.K, i);
        else msig_delin_item(P, i, lane_ws);
    }
    for (size_t t = 0; t < B; ++t) mv_sum_item(V, (uint32_t)t);
    if (verify) {
        unsigned long long tl[4] = {0, 0, 0, 0};
        run(params_single(u, r, agg.p(), m, B, g_comb_g.data(), out_ptrs{status, tl, nullptr, nullptr}));
        if (tally) for (int i = 0; i < 4; ++i) tally[i] = tl[i];
        for (size_t t = 0; t < B; ++t) mv_clear_item(V, (uint32_t)t);
    }
    memcpy(agg_pk, agg.p(), B * 64);
    return 0;
}

}  // extern "C"

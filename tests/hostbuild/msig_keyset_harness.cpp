// CPU build of csrc/msig_keyset.h (the multisignature call against a registered key set) for tests/test_msig_keyset_host.py:
// a set is registered with the functions the device runs at registration (kt_chain_key for the flags and the chains of bases,
// kt_table_lane for the window tables of the valid keys; the tables of the others stay zero-filled), a call runs the passes one
// item after the other in the order the device launches them.  The comb table and the CPU build of the inline passes
// (jjs_host_multisig) come from host_harness.cpp.
#include "host_harness.cpp"
#include "msig_keyset.h"

extern "C" {

// keys: n_keys x 64 affine; key_idx: N x uint32; z: N x 32; R, S: N x 64; m: B x 32; offsets: B + 1.  key_status: n_keys bytes out.
int jjs_msig_keyset_host_combine(const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R,
                                 const uint8_t* S, const uint8_t* m, const uint32_t* offsets, size_t B, uint8_t* key_status,
                                 uint8_t* share_status, uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    if (!keys || n_keys == 0 || n_keys > KEYSET_MAX_KEYS) return -1;
    ensure_tables();
    auto aligned = [](std::vector<uint32_t>& v) { return (uint32_t*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); };
    const int w = KEYSET_WINDOW;
    // ---- registration ----
    std::vector<uint32_t> key_item(n_keys), bases(n_keys * (size_t)kt_positions(w) * KT_BASE_WORDS + 4),
        tables(n_keys * (size_t)kt_positions(w) * kt_table_words(w) + 4, 0u), key_bytes(n_keys * 16 + 4);
    std::vector<uint8_t> flags(n_keys, 0);
    uint8_t* kb = (uint8_t*)aligned(key_bytes);
    memcpy(kb, keys, n_keys * 64);
    key_column C{};
    C.src = fe_src{kb, 64, 0};
    C.key_item = key_item.data(); C.key_flags = flags.data(); C.bases = aligned(bases); C.tables = aligned(tables);
    for (uint32_t id = 0; id < n_keys; ++id) {
        key_item[id] = id;
        if (kt_chain_key(C, id, w))
            for (uint32_t pos = 0; pos < (uint32_t)kt_positions(w); ++pos) kt_table_lane(C, id, pos, w);
        key_status[id] = (uint8_t)ks_key_status(flags[id], KT_KEY_VALID);
    }
    // ---- the call ----
    const size_t n = offsets[B];
    std::vector<uint32_t> tr(n + 1), d(8 * n + 8), dpk(EXT_WORDS * n + 4), ept(EXT_WORDS * n + 4), a(8 * B + 8), c(8 * B + 8),
        ws(WS_WORDS_PER_LANE + 4), long_tags(18 * B + 18, 0u), pk_col(16 * n + 8), row_key(n + 1), refused(B + 1, 0u);
    msig_keyset_params K{};
    msig_params& P = K.M;
    P.z = z; P.R = R; P.S = S; P.m = m; P.offsets = offsets; P.n_transcripts = (uint32_t)B; P.n_total = n;
    P.share_status = share_status; P.agg_pk = agg_pk; P.sig_u = sig_u; P.sig_R = sig_R; P.transcript_status = transcript_status;
    P.tr_of = tr.data(); P.d_words = d.data(); P.dpk = dpk.data(); P.e_pt = ept.data(); P.a_words = a.data(); P.c_words = c.data();
    P.tags = &JJS_SPONGE_TAG_LONG[0][0]; P.comb_g = g_comb_g.data();
    P.max_table_participants = JJS_MSIG_MAX_PARTICIPANTS;
    P.long_tags = long_tags.data();
    K.key_idx = key_idx; K.n_keys = (uint32_t)n_keys;
    K.keys = kb; K.flags = flags.data(); K.tables = C.tables;
    K.pk_col = (uint8_t*)aligned(pk_col); K.row_key = row_key.data(); K.refused = refused.data();
    P.PK = K.pk_col;
    uint32_t* lane_ws = aligned(ws);
    for (size_t t = 0; t < B; ++t) msig_map_item(P, (uint32_t)t);
    for (size_t i = 0; i < n; ++i) mk_gather_item(K, i);
    for (size_t i = 0; i < n; ++i) mk_delin_item(K, i);
    for (size_t t = 0; t < B; ++t) msig_agg_item(P, (uint32_t)t);
    for (size_t i = 0; i < n; ++i) msig_commit_item(P, i, lane_ws);
    for (size_t t = 0; t < B; ++t) msig_final_item(P, (uint32_t)t);
    for (size_t i = 0; i < n; ++i) mk_share_item(K, i);
    for (size_t t = 0; t < B; ++t) msig_verdict_item(P, (uint32_t)t);
    for (size_t t = 0; t < B; ++t) mk_refuse_item(K, (uint32_t)t);
    return 0;
}

}  // extern "C"

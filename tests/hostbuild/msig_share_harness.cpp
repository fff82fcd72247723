// CPU build of csrc/msig_share.h (verify_share on its own) for tests/test_msig_share_host.py: the three routes, the stage functions
// one item after the other in the order the device launches them -- the ingest of an extended or wire call in poison mode, the
// front of the route's combine call, the check pass over cleared flags, the sums pass, the two steps of the query pass.  A signer
// group and a key set are registered with the functions the device runs at registration, as msig_group_harness.cpp and
// msig_keyset_harness.cpp do.  The comb table, ext_normalize and host_dlog come from the harnesses included here.
#include "msig_ext_harness.cpp"
#include "msig_share.h"

extern "C" {

// route 0 (inline): keys = the PK column, N rows in format fmt.  route 1 (signer group): keys = the group's n_keys affine keys, a
// transcript has n_keys rows, offsets is not read.  route 2 (key set): keys = the set's n_keys affine keys, key_idx N x uint32.
// fmt (0 affine, 1 extended, 2 wire) describes R, S and the inline PK column; lanes: the launch shape of the ingest.  m: B x 32;
// qt, qs: Q x uint32; z: Q x 32; status: Q bytes; sig_R: B x 64 or NULL.  Every pointer is 16-byte aligned.
int jjs_msig_share_host(int route, int fmt, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* R, const uint8_t* S,
                        const uint8_t* m, const uint32_t* offsets, size_t B, size_t lanes, const uint32_t* qt, const uint32_t* qs,
                        const uint8_t* z, size_t Q, uint8_t* status, uint8_t* sig_R) {
    if (route < 0 || route > 2 || fmt < 0 || fmt > 2 || lanes == 0) return -1;
    if (route == 1 && !mg_keys_acceptable(keys, n_keys)) return -1;
    ensure_tables();
    auto aligned = [](std::vector<uint32_t>& v) { return (uint32_t*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); };
    const size_t n = route == 1 ? B * n_keys : offsets[B];
    // ---- ingest ----
    column c0(n + 1), c1(n + 1), c2(n + 1), agg(B + 1), rsa(B + 1);
    const uint8_t* pts[3] = {keys, R, S};
    uint8_t* out[3] = {c0.p(), c1.p(), c2.p()};
    const int first = route == 0 ? 0 : 1, k = 3 - first;
    if (fmt == 1 && n) {
        ext_normalize(pts + first, (uint32_t)k, n, lanes, 1, out + first, nullptr);
    } else if (fmt == 2 && n) {
        msig_decode_params D{};
        D.n_src = (uint32_t)k; D.n = n; D.dlog = host_dlog();
        for (int i = 0; i < k; ++i) { D.src[i] = fe_src{pts[first + i], 32, 0}; D.out[i] = out[first + i]; }
        for (size_t lane = 0; lane < lanes; ++lane) msig_decode_lane(D, lane, lanes);
    }
    if (fmt != 0 && n)
        for (int i = first; i < 3; ++i) pts[i] = out[i];
    // ---- the call ----
    std::vector<uint32_t> tr(n + 1), d(8 * n + 8), dpk(EXT_WORDS * n + 4), qpt(EXT_WORDS * Q + 4), a(8 * B + 8), c(8 * B + 8),
        ws(WS_WORDS_PER_LANE + 4), long_tags(18 * B + 18, 0u), bad(B + 1, 0u), pk_col(16 * n + 8), row_key(n + 1);
    uint32_t* w = aligned(ws);
    msig_share_params X{};
    msig_params& P = X.M;
    P.R = pts[1]; P.S = pts[2]; P.m = m; P.offsets = offsets; P.n_transcripts = (uint32_t)B; P.n_total = n;
    P.agg_pk = agg.p(); P.sig_R = sig_R ? sig_R : rsa.p();
    P.tr_of = tr.data(); P.d_words = d.data(); P.dpk = dpk.data(); P.e_pt = qpt.data(); P.a_words = a.data(); P.c_words = c.data();
    P.tags = &JJS_SPONGE_TAG_LONG[0][0]; P.comb_g = g_comb_g.data();
    P.max_table_participants = JJS_MSIG_MAX_PARTICIPANTS;
    P.long_tags = long_tags.data();
    X.q_transcript = qt; X.q_slot = qs; X.q_z = z; X.n_queries = Q; X.q_status = status;
    X.bad = bad.data(); X.d_words = d.data();
    // (registered objects live to the end of the call)
    std::vector<uint32_t> g_tr, g_d, g_dpk, g_tags, bases, tables, key_item, key_bytes;
    std::vector<uint8_t> flags;
    if (route == 0) {
        P.PK = pts[0];
        X.check_pk = 1;
        for (size_t t = 0; t < B; ++t) msig_map_item(P, (uint32_t)t);
        for (size_t i = 0; i < n; ++i) msig_delin_item(P, i, w);
        for (size_t t = 0; t < B; ++t) msig_agg_item(P, (uint32_t)t);
    } else if (route == 1) {
        const size_t gn = n_keys;
        g_tr.assign(gn, 0u); g_d.resize(8 * gn); g_dpk.resize(EXT_WORDS * gn); g_tags.resize(18);
        bases.resize(gn * MG_BASE_WORDS_PER_KEY + 4); tables.resize(gn * MG_TABLE_WORDS_PER_KEY + 4);
        const uint32_t g_off[2] = {0, (uint32_t)gn};
        for (int which = 0; which < 2; ++which) {
            const uint32_t n_in = which ? 3u + 4u * (uint32_t)gn : 2u + 2u * (uint32_t)gn;
            if (gn <= JJS_MSIG_MAX_PARTICIPANTS) memcpy(&g_tags[9 * which], JJS_SPONGE_TAG_LONG[n_in], 36);
            else safe_tag_limbs(n_in, JJS_Q_WORDS, &g_tags[9 * which]);
        }
        msig_params Gp{};
        Gp.PK = keys; Gp.offsets = g_off; Gp.n_transcripts = 1; Gp.n_total = gn;
        Gp.tr_of = g_tr.data(); Gp.d_words = g_d.data(); Gp.dpk = g_dpk.data();
        Gp.long_tags = g_tags.data(); Gp.max_table_participants = 0;
        for (size_t i = 0; i < gn; ++i) msig_delin_item(Gp, i, w);
        store_point(agg.p(), 0, sum_points_affine(g_dpk.data(), 0, (uint32_t)gn));
        uint32_t *b = aligned(bases), *t = aligned(tables);
        for (uint32_t j = 0; j < gn; ++j) {
            mg_chain_item(keys, j, b);
            for (uint32_t pos = 0; pos < (uint32_t)kt_positions(MG_WINDOW); ++pos) mg_table_item(b, t, j, pos);
        }
        X.participants = (uint32_t)gn; X.d_words = g_d.data(); X.tables = t; X.tag_a = &g_tags[9];
        msig_group_params G{};
        G.M = P; G.participants = X.participants; G.d_words = X.d_words; G.tables = X.tables; G.tag_a = X.tag_a;
        for (size_t t_i = 0; t_i < B; ++t_i) mg_binding_item(G, (uint32_t)t_i);
    } else {
        if (!keys || n_keys == 0 || n_keys > KEYSET_MAX_KEYS) return -1;
        const int kw = KEYSET_WINDOW;
        key_item.resize(n_keys); bases.resize(n_keys * (size_t)kt_positions(kw) * KT_BASE_WORDS + 4);
        tables.assign(n_keys * (size_t)kt_positions(kw) * kt_table_words(kw) + 4, 0u); key_bytes.resize(n_keys * 16 + 4);
        flags.assign(n_keys, 0);
        uint8_t* kb = (uint8_t*)aligned(key_bytes);
        memcpy(kb, keys, n_keys * 64);
        key_column C{};
        C.src = fe_src{kb, 64, 0};
        C.key_item = key_item.data(); C.key_flags = flags.data(); C.bases = aligned(bases); C.tables = aligned(tables);
        for (uint32_t id = 0; id < n_keys; ++id) {
            key_item[id] = id;
            if (kt_chain_key(C, id, kw))
                for (uint32_t pos = 0; pos < (uint32_t)kt_positions(kw); ++pos) kt_table_lane(C, id, pos, kw);
        }
        msig_keyset_params K{};
        P.PK = (uint8_t*)aligned(pk_col);
        K.M = P;
        K.key_idx = key_idx; K.n_keys = (uint32_t)n_keys;
        K.keys = kb; K.flags = flags.data(); K.tables = C.tables;
        K.pk_col = (uint8_t*)aligned(pk_col); K.row_key = row_key.data(); K.refused = bad.data();
        X.tables = C.tables; X.row_key = row_key.data();
        for (size_t t = 0; t < B; ++t) msig_map_item(P, (uint32_t)t);
        for (size_t i = 0; i < n; ++i) mk_gather_item(K, i);
        for (size_t i = 0; i < n; ++i) mk_delin_item(K, i);
        for (size_t t = 0; t < B; ++t) msig_agg_item(P, (uint32_t)t);
    }
    for (size_t i = 0; i < n; ++i) msh_check_item(X, i);
    for (size_t t = 0; t < B; ++t) msh_sums_item(X, (uint32_t)t, w);
    for (size_t q = 0; q < Q; ++q) msh_commit_item(X, q, w);
    for (size_t q = 0; q < Q; ++q) {
        if (route == 0) msh_inline_item(X, q, w);
        else msh_tables_item(X, q);
    }
    return 0;
}

}  // extern "C"

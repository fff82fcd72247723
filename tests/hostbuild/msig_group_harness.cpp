// CPU build of csrc/msig_group.h (multisig signer groups) for tests/test_msig_group_host.py: a group is registered with the
// functions the device runs at registration (msig_delin_item over a one-transcript descriptor, sum_points_affine,
// mg_chain_item, mg_table_item), a call runs the five passes one item after the other, pass 3 in either lane order.
// The comb table and the other CPU entry points come from host_harness.cpp.
#include "host_harness.cpp"
#include "msig_group.h"

extern "C" {

// what jjs_msig_group_create checks before it builds anything: 0 acceptable, -1 refused
int jjs_msig_group_host_check(const uint8_t* PK, size_t n) { return mg_keys_acceptable(PK, n) ? 0 : -1; }

// PK: n x 64 (the ordered key vector); z: B n x 32; R, S: B n x 64; m: B x 32.  by_participant: the lane order of pass 3.
int jjs_msig_group_host_combine(const uint8_t* PK, size_t n, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m, size_t B,
                                int by_participant, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R,
                                uint8_t* agg_pk) {
    if (!mg_keys_acceptable(PK, n)) return -1;
    if ((uint64_t)B * n >= (1ull << 32)) return -1;
    ensure_tables();
    auto aligned = [](std::vector<uint32_t>& v) { return (uint32_t*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); };
    // ---- registration ----
    std::vector<uint32_t> tr(n, 0u), d(8 * n), dpk(EXT_WORDS * n), ws(WS_WORDS_PER_LANE + 4), tags(18), bases(n * MG_BASE_WORDS_PER_KEY + 4),
        tables(n * MG_TABLE_WORDS_PER_KEY + 4), agg(16 + 4);
    const uint32_t offsets[2] = {0, (uint32_t)n};
    for (int which = 0; which < 2; ++which) {
        const uint32_t n_in = which ? 3u + 4u * (uint32_t)n : 2u + 2u * (uint32_t)n;
        if (n <= JJS_MSIG_MAX_PARTICIPANTS) memcpy(&tags[9 * which], JJS_SPONGE_TAG_LONG[n_in], 36);
        else safe_tag_limbs(n_in, JJS_Q_WORDS, &tags[9 * which]);
    }
    uint32_t* w = aligned(ws);
    msig_params P{};
    P.PK = PK; P.offsets = offsets; P.n_transcripts = 1; P.n_total = n;
    P.tr_of = tr.data(); P.d_words = d.data(); P.dpk = dpk.data();
    P.long_tags = tags.data(); P.max_table_participants = 0;
    for (size_t i = 0; i < n; ++i) msig_delin_item(P, i, w);
    uint8_t* agg_bytes = (uint8_t*)aligned(agg);
    store_point(agg_bytes, 0, sum_points_affine(dpk.data(), 0, (uint32_t)n));
    memcpy(agg_pk, agg_bytes, 64);
    uint32_t *b = aligned(bases), *t = aligned(tables);
    for (uint32_t j = 0; j < n; ++j) {
        mg_chain_item(PK, j, b);
        for (uint32_t pos = 0; pos < (uint32_t)kt_positions(MG_WINDOW); ++pos) mg_table_item(b, t, j, pos);
    }
    // ---- the call ----
    const size_t N = B * n;
    std::vector<uint32_t> ept(EXT_WORDS * N + 4), a(8 * B + 4), c(8 * B + 4);
    msig_group_params G{};
    msig_params& M = G.M;
    M.z = z; M.R = R; M.S = S; M.m = m; M.n_transcripts = (uint32_t)B; M.n_total = N;
    M.share_status = share_status; M.transcript_status = transcript_status; M.sig_u = sig_u; M.sig_R = sig_R; M.agg_pk = agg_bytes;
    M.e_pt = ept.data(); M.a_words = a.data(); M.c_words = c.data(); M.comb_g = g_comb_g.data();
    G.participants = (uint32_t)n; G.by_participant = by_participant ? 1u : 0u;
    G.d_words = d.data(); G.tables = t; G.tag_a = &tags[9];
    for (size_t tr_i = 0; tr_i < B; ++tr_i) mg_binding_item(G, (uint32_t)tr_i);
    for (size_t i = 0; i < N; ++i) mg_commit_item(G, i, w);
    for (size_t tr_i = 0; tr_i < B; ++tr_i) mg_final_item(G, (uint32_t)tr_i);
    std::vector<uint8_t> seen(N, 0);
    for (size_t k = 0; k < N; ++k) {
        const uint64_t i = mg_share_of_lane(G, k);
        if (i >= N || seen[i]) return -3;          // the lane order is a permutation of the shares
        seen[i] = 1;
        mg_share_item(G, i);
    }
    for (size_t tr_i = 0; tr_i < B; ++tr_i) mg_verdict_item(G, (uint32_t)tr_i);
    return 0;
}

}  // extern "C"

// CPU build of csrc/msig_sign.h (the signer's half of the multisignature scheme) for tests/test_msig_sign_host.py: the passes one
// item after the other in the order the device launches them -- normalize_lane in poison mode for an extended call, the map, the
// check pass over cleared flags, the delinearisation, the aggregate key and a, the commitments, ms_final_item, the share pass --
// and sign_round_1.  The comb table and ext_normalize come from host_harness.cpp and msig_ext_harness.cpp.
#include "msig_ext_harness.cpp"
#include "msig_sign.h"

extern "C" {

// PK, R, S: N x 64 / N x 96 (ext); m: B x 32; signer_row: n_signing x uint32 or NULL (then n_signing == N); sk, r, s: n_signing x 32.
// lanes: the launch shape of the normalisation.  Every pointer is 16-byte aligned.
int jjs_msig_sign_host(int ext, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m, const uint32_t* offsets, size_t B,
                       size_t lanes, const uint32_t* signer_row, const uint8_t* sk, const uint8_t* r, const uint8_t* s, size_t n_signing,
                       uint8_t* z_out, uint8_t* status) {
    ensure_tables();
    const size_t n = offsets[B];
    if (!signer_row && n_signing != n) return -1;
    column pk(n + 1), rr(n + 1), ss(n + 1), agg(B + 1), rsa(B + 1);
    const uint8_t* pts[3] = {PK, R, S};
    if (ext && n) {
        uint8_t* out[3] = {pk.p(), rr.p(), ss.p()};
        ext_normalize(pts, 3, n, lanes, 1, out, nullptr);
        for (int k = 0; k < 3; ++k) pts[k] = out[k];
    }
    std::vector<uint32_t> tr(n + 1), d(8 * n + 8), dpk(EXT_WORDS * n + 4), ept(EXT_WORDS * n + 4), a(8 * B + 8), c(8 * B + 8), ws(WS_WORDS_PER_LANE + 4),
        long_tags(18 * B + 18, 0u), flags(n + 2 * B + 1, 0u);
    msig_sign_params G{};
    msig_params& P = G.M;
    P.PK = pts[0]; P.R = pts[1]; P.S = pts[2]; P.m = m; P.offsets = offsets; P.n_transcripts = (uint32_t)B; P.n_total = n;
    P.agg_pk = agg.p(); P.sig_R = rsa.p();
    P.tr_of = tr.data(); P.d_words = d.data(); P.dpk = dpk.data(); P.e_pt = ept.data(); P.a_words = a.data(); P.c_words = c.data();
    P.tags = &JJS_SPONGE_TAG_LONG[0][0]; P.comb_g = g_comb_g.data();
    P.max_table_participants = JJS_MSIG_MAX_PARTICIPANTS;
    P.long_tags = long_tags.data();
    G.pk_repeats = flags.data(); G.bad_enc = flags.data() + n; G.dup_nonce = G.bad_enc + B;
    G.signer_row = signer_row; G.sk = sk; G.r = r; G.s = s; G.n_signing = n_signing; G.z_out = z_out; G.status = status;
    uint32_t* w = (uint32_t*)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
    for (size_t t = 0; t < B; ++t) msig_map_item(P, (uint32_t)t);
    for (size_t i = 0; i < n; ++i) ms_check_item(G, i);
    for (size_t i = 0; i < n; ++i) msig_delin_item(P, i, w);
    for (size_t t = 0; t < B; ++t) msig_agg_item(P, (uint32_t)t);
    for (size_t i = 0; i < n; ++i) msig_commit_item(P, i, w);
    for (size_t t = 0; t < B; ++t) ms_final_item(P, (uint32_t)t);
    for (size_t j = 0; j < n_signing; ++j) ms_share_item(G, j);
    return 0;
}

int jjs_msig_sign_host_round1(const uint8_t* r, const uint8_t* s, size_t n, uint8_t* R_out, uint8_t* S_out, uint8_t* bad) {
    ensure_tables();
    for (size_t i = 0; i < n; ++i) ms_round1_item(r, s, g_comb_g.data(), i, R_out, S_out, bad);
    return 0;
}

}  // extern "C"

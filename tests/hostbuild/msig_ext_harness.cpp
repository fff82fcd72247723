// CPU build of the extended-coordinate multisignature calls for tests/test_msig_ext_host.py: normalize_lane in poison mode
// (csrc/normalize.h) in front of the CPU build of the passes, as the *_ext entry points queue msig_normalize_kernel in front
// of pass 0 -- a share row as one item of three sources, a group call's row as one of two, a registration as one column.
// `lanes` is the launch shape: a lane owns the rows lane, lane + lanes, ...  The passes, the signer groups and the comb
// table come from msig_group_harness.cpp and host_harness.cpp.
#include "msig_group_harness.cpp"

// k columns of n x 96 -> k columns of n x 64; poison = 0 is the verify paths' mode (flags in `bad`, nullable)
static void ext_normalize(const uint8_t* const* ext, uint32_t k, size_t n, size_t lanes, int poison, uint8_t* const* out, uint8_t* bad) {
    std::vector<uint32_t> scratch(9 * n + 16);
    normalize_params P{};
    P.n_src = k; P.poison = poison ? 1u : 0u; P.n = n; P.bad = bad; P.scratch = scratch.data();
    for (uint32_t i = 0; i < k; ++i) { P.src[i] = fe_src{ext[i], 96, 0}; P.out[i] = out[i]; }
    for (size_t lane = 0; lane < lanes; ++lane) {
        if (poison) normalize_lane<true>(P, lane, lanes);
        else normalize_lane(P, lane, lanes);
    }
}
// 16-byte aligned n x 64 column
struct column {
    std::vector<u32x4> v;
    explicit column(size_t n) : v(4 * n + 1) {}
    uint8_t* p() { return reinterpret_cast<uint8_t*>(v.data()); }
};

extern "C" {

int jjs_msig_ext_host_normalize(const uint8_t* const* ext, int k, size_t n, size_t lanes, int poison, uint8_t* const* out, uint8_t* bad) {
    if (bad) memset(bad, 0, n);
    ext_normalize(ext, (uint32_t)k, n, lanes, poison, out, bad);
    return 0;
}
int jjs_msig_ext_host_check(const uint8_t* PK_ext, size_t n) { return mg_ext_keys_usable(PK_ext, n) ? 0 : -1; }

int jjs_msig_ext_host_combine(const uint8_t* z, const uint8_t* PK_ext, const uint8_t* R_ext, const uint8_t* S_ext, const uint8_t* m,
                              const uint32_t* offsets, size_t B, size_t lanes, uint8_t* status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R,
                              uint8_t* transcript_status) {
    const size_t n = offsets[B];
    column pk(n), r(n), s(n);
    const uint8_t* ext[3] = {PK_ext, R_ext, S_ext};
    uint8_t* out[3] = {pk.p(), r.p(), s.p()};
    ext_normalize(ext, 3, n, lanes, 1, out, nullptr);
    return jjs_host_multisig(z, pk.p(), r.p(), s.p(), m, offsets, B, status, agg_pk, sig_u, sig_R, transcript_status);
}
int jjs_msig_ext_host_group_combine(const uint8_t* PK_ext, size_t n, const uint8_t* z, const uint8_t* R_ext, const uint8_t* S_ext, const uint8_t* m,
                                    size_t B, size_t lanes, int by_participant, uint8_t* status, uint8_t* transcript_status, uint8_t* sig_u,
                                    uint8_t* sig_R, uint8_t* agg_pk) {
    if (!mg_ext_keys_usable(PK_ext, n)) return -1;
    column pk(n), r(n * B), s(n * B);
    uint8_t* kout[1] = {pk.p()};
    ext_normalize(&PK_ext, 1, n, lanes, 1, kout, nullptr);
    const uint8_t* ext[2] = {R_ext, S_ext};
    uint8_t* out[2] = {r.p(), s.p()};
    ext_normalize(ext, 2, n * B, lanes, 1, out, nullptr);
    return jjs_msig_group_host_combine(pk.p(), n, z, r.p(), s.p(), m, B, by_participant, status, transcript_status, sig_u, sig_R, agg_pk);
}

}  // extern "C"

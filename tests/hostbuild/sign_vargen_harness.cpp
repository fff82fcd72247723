// CPU build of csrc/sign_vargen.h (var-generator signing and key derivation with the generator as a point) for
// tests/test_sign_vargen_pt_host.py: the front as the device queues it -- normalize_lane in poison mode for an extended generator
// column, msig_decode_lane for a wire one, `lanes` the launch shape -- and then the item body one item after the other over the
// derived affine column.  route 1 is the shared-generator route: the window tables of generator row 0 built by the CPU build of the
// table functions (mg_chain_item, mg_table_item), then the tabled item body.  ext_normalize and the square-root tables come from msig_ext_harness.cpp and host_harness.cpp.
#include "msig_ext_harness.cpp"
#include "sign_vargen.h"

extern "C" {

// route 0: the per-item route; 1: the shared-generator route (signing, n_gen == 1).  format 0 / 1 / 2: Gen is n_gen x 64 / 96 / 32; n_gen is n or 1.  sign = 0: the derivation (rnd, m, u_out, R_out unused).
// PK_out (when signing) and Gen_out may be NULL.  Every pointer but status is 16-byte aligned.
int jjs_sign_vargen_host(int format, int sign, int route, const uint8_t* sk, const uint8_t* Gen, size_t n_gen, const uint8_t* rnd, const uint8_t* m, size_t n,
                         size_t lanes, uint8_t* u_out, uint8_t* R_out, uint8_t* PK_out, uint8_t* Gen_out, uint8_t* status) {
    if (format < 0 || format > 2 || (n_gen != n && n_gen != 1) || lanes == 0 || (route && (!sign || n_gen != 1))) return -1;
    if (n == 0) return 0;
    column derived(n_gen + 1);
    const uint8_t* gen = Gen;
    if (format == 1) {
        uint8_t* out[1] = {derived.p()};
        ext_normalize(&Gen, 1, n_gen, lanes, 1, out, nullptr);
        gen = derived.p();
    } else if (format == 2) {
        msig_decode_params D{};
        D.n_src = 1; D.n = n_gen; D.dlog = host_dlog();
        D.src[0] = fe_src{Gen, 32, 0}; D.out[0] = derived.p();
        for (size_t lane = 0; lane < lanes; ++lane) msig_decode_lane(D, lane, lanes);
        gen = derived.p();
    }
    std::vector<uint32_t> ws(WS_WORDS_PER_LANE + 4);
    uint32_t* w = (uint32_t*)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
    sign_vargen_params P{};
    P.sk = sk; P.gen = gen; P.rnd = rnd; P.m = m;
    P.gen_stride = (n_gen == 1 && n > 1) ? 0u : 64u;
    P.u_out = u_out; P.R_out = R_out; P.PK_out = PK_out; P.Gen_out = Gen_out; P.status = status; P.n = n; P.workspace = w;
    std::vector<u32x4> bases(MG_BASE_WORDS_PER_KEY / 4 + 1), tables(MG_TABLE_WORDS_PER_KEY / 4 + 1);
    if (route) {
        mg_chain_item(gen, 0, reinterpret_cast<uint32_t*>(bases.data()));
        for (int pos = 0; pos < kt_positions(MG_WINDOW); ++pos)
            mg_table_item(reinterpret_cast<const uint32_t*>(bases.data()), reinterpret_cast<uint32_t*>(tables.data()), 0, (uint32_t)pos);
        P.tables = reinterpret_cast<const uint32_t*>(tables.data());
    }
    for (size_t i = 0; i < n; ++i) {
        if (route) sign_vargen_item<true, true>(P, i, w);
        else if (sign) sign_vargen_item<true>(P, i, w);
        else sign_vargen_item<false>(P, i, w);
    }
    return 0;
}

}  // extern "C"

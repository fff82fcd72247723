// CPU build of csrc/sign_fixed.h (signing and key derivation with a SecretKey, single and double scheme) for
// tests/test_sign_fixed_host.py: the item bodies one item after the other, as the device's lanes run them, and in front of the
// keyed body the pre-pass, as the device's one-lane launch runs it.  The comb tables come from host_harness.cpp.
#include "msig_ext_harness.cpp"
#include "sign_fixed.h"

extern "C" {

// scheme 0 single / 1 double.  sign = 0: the derivation (n_sk = n; rnd, m and the signature outputs unused).  route 0: the per-item
// body (n_sk == 1 and n > 1: the key row read with stride 0); route 1: the pre-pass and the keyed body (signing, n_sk == 1, any n).
// Every output but status may be NULL.  Every pointer but status is 16-byte aligned.
int jjs_sign_fixed_host(int scheme, int sign, int route, const uint8_t* sk, size_t n_sk, const uint8_t* rnd, const uint8_t* m, size_t n,
                        uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out, uint8_t* PK_out, uint8_t* PKp_out, uint8_t* sig_w, uint8_t* pk_w,
                        uint8_t* status) {
    if (scheme < 0 || scheme > 1 || (n_sk != n && n_sk != 1) || (route && (!sign || n_sk != 1))) return -1;
    if (n == 0) return 0;
    ensure_tables();
    std::vector<uint32_t> ws(WS_WORDS_PER_LANE + 4);
    uint32_t* w = (uint32_t*)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
    std::vector<u32x4> key(SF_KEY_WORDS / 4);
    sign_fixed_params P{};
    P.sk = sk; P.rnd = rnd; P.m = m;
    P.sk_stride = (n_sk == 1 && n > 1) ? 0u : 32u;
    P.u_out = u_out; P.R_out = R_out; P.Rp_out = Rp_out; P.PK_out = PK_out; P.PKp_out = PKp_out; P.sig_w = sig_w; P.pk_w = pk_w;
    P.status = status; P.comb_g = g_comb_g.data(); P.comb_gn = g_comb_gn.data(); P.n = n; P.workspace = w;
    if (route) {
        P.key = reinterpret_cast<uint32_t*>(key.data());
        if (scheme) sign_fixed_key<true>(P); else sign_fixed_key<false>(P);
    }
    for (size_t i = 0; i < n; ++i) {
        if (!sign) { if (scheme) derive_fixed_item<true>(P, i); else derive_fixed_item<false>(P, i); }
        else if (route) { if (scheme) sign_fixed_item<true, true>(P, i, w); else sign_fixed_item<false, true>(P, i, w); }
        else if (scheme) sign_fixed_item<true, false>(P, i, w);
        else sign_fixed_item<false, false>(P, i, w);
    }
    return 0;
}

}  // extern "C"

// Var-generator signing and key derivation with the generator given as a POINT (include/jjs_gpu.h jjs_sign_vargen_pt*,
// jjs_public_keys_vargen*): what a caller holds who has a SecretKeyVarGen as the reference builds and serialises it,
//   SecretKeyVarGen { sk, generator }   reference src/keys/secret/var_gen.rs:98-101, new :147, from_bytes :109-131
//   PublicKeyVarGen::from(&sk)          pk = sk * generator
//   SecretKeyVarGen::sign               src/keys/secret/var_gen.rs:228-256, nonce src/nonce.rs:68-85
// where the generator has no known discrete logarithm (sign_core.h's sign_item takes a scalar and signs under gen_scalar * G).
// A generator of test and benchmark material like every signer here, NOT constant time (table look-ups and branches depend on
// the secret key and the nonce): never use with production keys.
//
// One lane per item.  The lane's workspace holds the 4-bit table of the generator and the transcript area, as sign_item's.  The
// item is range-tested (sk, rnd < r; m and the generator's coordinates < q) and the generator is tested for the curve equation
// (the test jjs_multisig_verify applies to inline keys: the addition law is only an addition law on the curve); nothing else is
// validated, as in the reference -- the identity, small-order points, points with a torsion part and sk = 0 sign and derive.  A
// refused item gets status 3 and zero bytes in every output row.  R = r * Gen and PK = sk * Gen share ONE field inversion
// (sign_item spends one each).  The generator column is affine: extended and wire generators were brought to it in poison mode
// (normalize.h, decode.h), where every unusable point is 64 bytes of 0xFF, which the range test here refuses.
//
// The shared-generator route (TABLED; a signing call with ONE generator for all its items): the 6-bit window tables of the
// generator, {0 .. 32} * 2^(6 i) * Gen for the 43 positions, are built once per call by the registration kernels of the signer
// groups (msig_group.h mg_chain_item, mg_table_item: every point is tabled, nothing is validated), and the lane replaces its
// table and the two chains of 252 doublings by two walks of 43 additions (kt_add_scalar).  Range tests, hashes, the shared
// inversion and every output are those of the per-item route: the two routes agree byte for byte on every point of the curve.
#pragma once
#include "msig_group.h"
#include "sign_core.h"

namespace jjs {

struct sign_vargen_params {
    const uint8_t *sk, *gen, *rnd, *m;   // gen: n x 64 affine, or one row read by every item (gen_stride 0)
    uint32_t gen_stride, pad_;           // 64: a generator per item; 0: one generator for the call
    uint8_t *u_out, *R_out, *PK_out, *Gen_out, *status;     // PK_out (of a signing call) and Gen_out may be null; status: bytes, any alignment
    uint64_t n;
    uint32_t* workspace;                 // WS_WORDS_PER_LANE words per resident lane
    const uint32_t* tables;              // the shared-generator route: MG_TABLE_WORDS_PER_KEY words, the window tables of gen row 0
};

// a generator as the calls accept it: both coordinates canonical, and on the curve
JJS_HD bool svg_generator_usable(const words8& u, const words8& v) {
    if (!words_lt(u, JJS_Q_WORDS) || !words_lt(v, JJS_Q_WORDS)) return false;
    return affine_on_curve(fq_from_words(u), fq_from_words(v));
}
JJS_HD void svg_store_zero_point(uint8_t* base, uint64_t item) {
    store_words(base, 2 * item, words_zero());
    store_words(base, 2 * item + 1, words_zero());
}
// R and PK in affine form with one inversion between them (Z is never zero: the addition law is complete)
JJS_HD void svg_two_affine(const ext_pt& a, const ext_pt& b, affine_words& A, affine_words& B) {
    const fe_n inv = fq_inverse(fq_mul(a.z, b.z));
    const fe_n ai = fq_mul(inv, b.z), bi = fq_mul(inv, a.z);
    A.u = fq_to_words(fq_mul(a.x, ai)); A.v = fq_to_words(fq_mul(a.y, ai));
    B.u = fq_to_words(fq_mul(b.x, bi)); B.v = fq_to_words(fq_mul(b.y, bi));
}

// SIGN: SecretKeyVarGen::sign given the RNG draw.  !SIGN: PublicKeyVarGen::from alone -- no hashes, no r; rnd, m, u_out and
// R_out are not touched.  TABLED: the multiplications walk P.tables (the shared-generator route) instead of a table built here.
// NOT constant time.
template <bool SIGN, bool TABLED = false>
JJS_HD void sign_vargen_item(const sign_vargen_params& P, uint64_t item, uint32_t* ws) {
    uint32_t* tab = ws;                    // the generator's table
    uint32_t* area = ws + TABLE_WORDS;     // transcript staging (second table's space)
    const fe_src s_sk{P.sk, 32, 0}, s_gen{P.gen, P.gen_stride, 0};
    const bool shared = P.gen_stride == 0;
    const words8 sk = load_words(s_sk, item);
    affine_words gen;
    gen.u = load_words(s_gen, item); gen.v = load_words(s_gen, item, 32);
    const bool gen_ok = svg_generator_usable(gen.u, gen.v);
    bool ok = gen_ok && words_lt(sk, JJS_FR_WORDS);
    words8 rnd = words_zero(), m = words_zero();
    if (SIGN) {
        const fe_src s_rnd{P.rnd, 32, 0}, s_m{P.m, 32, 0};
        rnd = load_words(s_rnd, item); m = load_words(s_m, item);
        ok = ok && words_lt(rnd, JJS_FR_WORDS) && words_lt(m, JJS_Q_WORDS);
    }
    // the canonical generator: one row per item, or one row for the call, which the lane of item 0 writes
    if (P.Gen_out && shared && item == 0) {
        if (gen_ok) store_point(P.Gen_out, 0, gen); else svg_store_zero_point(P.Gen_out, 0);
    }
    P.status[item] = (uint8_t)(ok ? (uint32_t)ST_OK : (uint32_t)ST_MALFORMED);
    if (!ok) {
        if (SIGN) { store_words(P.u_out, item, words_zero()); svg_store_zero_point(P.R_out, item); }
        if (P.PK_out) svg_store_zero_point(P.PK_out, item);
        if (P.Gen_out && !shared) svg_store_zero_point(P.Gen_out, item);
        return;
    }
    if (!TABLED) build_point_table(tab, fq_from_words(gen.u), fq_from_words(gen.v));
    key_column C{};
    C.tables = const_cast<uint32_t*>(P.tables);
    if (!SIGN) {
        store_point(P.PK_out, item, to_affine_words(table_mul(tab, sk)));
        if (P.Gen_out && !shared) store_point(P.Gen_out, item, gen);
        return;
    }
    stage(area, 0, rnd); stage(area, 1, sk); stage(area, 2, gen.u); stage(area, 3, gen.v); stage(area, 4, m);
    const words8 r = staged_digest(area, 5);
    affine_words R, PK;
    {
        const ext_pt rp = TABLED ? kt_add_scalar(ext_identity(), C, 0, r, MG_WINDOW) : table_mul(tab, r);
        svg_two_affine(rp, TABLED ? kt_add_scalar(ext_identity(), C, 0, sk, MG_WINDOW) : table_mul(tab, sk), R, PK);
    }
    stage(area, 0, R.u); stage(area, 1, R.v); stage(area, 2, PK.u); stage(area, 3, PK.v);
    stage(area, 4, gen.u); stage(area, 5, gen.v); stage(area, 6, m);
    const words8 c = staged_digest(area, 7);
    store_words(P.u_out, item, fr_sub_mul(r, c, sk));
    store_point(P.R_out, item, R);
    if (P.PK_out) store_point(P.PK_out, item, PK);
    if (P.Gen_out && !shared) store_point(P.Gen_out, item, gen);
}

}  // namespace jjs

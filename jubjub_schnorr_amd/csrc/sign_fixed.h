// Signing and key derivation with a SecretKey in the single and the double scheme (include/jjs_gpu.h jjs_sign_fixed*,
// jjs_public_keys_fixed*): what a caller holds who has a SecretKey as the reference builds and serialises it,
//   SecretKey::from_bytes, sign      reference src/keys/secret.rs:103-194, nonce src/nonce.rs:32-44
//   SecretKey::sign_double           src/keys/secret/double.rs:56-85, nonce src/nonce.rs:49-61
//   PublicKey::from(&sk)             src/keys/public.rs:54-60          pk = sk * G
//   PublicKeyDouble::from(&sk)       src/keys/public/double.rs:47-57   (sk * G, sk * G')
// The arithmetic is sign_core.h's sign_item, value for value; what differs is around it.  A generator of test and benchmark
// material like every signer here, NOT constant time (table look-ups and branches depend on the secret key and the nonce): never
// use with production keys.
//
// One lane per item.  The lane's workspace holds the transcript area, as sign_item's.  The item is range-tested first (sk, rnd < r;
// m < q); nothing else is validated, as in the reference -- sk = 0 signs, and its key is the identity.  A refused item gets status 3
// and zero bytes in every output row it owns.  All the points of an item share ONE field inversion (sign_item spends one per
// point): R and PK; R, R', PK and PK' in the double scheme.  Besides the affine columns an item writes the wire rows a signer
// sends, Signature::to_bytes (u || compress(R) [|| compress(R')]) and PublicKey::to_bytes (compress(PK) [|| compress(PK')]).
//
// One key for the call (sk_stride 0: sk is one row, and so are the key outputs).  The key rows belong to the call, not to an item:
// they are the key's whatever the items' rnd and m are, and zero when the key is unusable, which also refuses every item.
//   per-item route   every lane reads sk row 0 and multiplies it out again; the lane of item 0 writes the key rows.
//   keyed route      (KEYED) sign_fixed_key, on one lane of a launch in front, range-tests the key, derives PK (and PK') with one
//                    inversion and leaves the canonical affine point(s), their wire form and a usable flag in a record of
//                    SF_KEY_WORDS words, and writes the key rows.  The lanes read PK from the record and run only r * G (and
//                    r * G'): their one inversion covers one or two points.
// Both routes give the same bytes.  A call of one item owns its key row like any item of a key-per-item call.
#pragma once
#include "sign_vargen.h"

namespace jjs {

struct sign_fixed_params {
    const uint8_t *sk, *rnd, *m;         // sk: n x 32, or one row read by every item (sk_stride 0)
    uint32_t sk_stride, pad_;            // 32: a key per item; 0: one key for the call
    uint8_t *u_out, *R_out, *Rp_out, *PK_out, *PKp_out, *sig_w, *pk_w, *status;   // every output but status may be null
    const uint32_t *comb_g, *comb_gn;
    uint64_t n;
    uint32_t* workspace;                 // WS_WORDS_PER_LANE words per resident lane
    uint32_t* key;                       // the keyed route: the record of sign_fixed_key
};

// the record of the keyed route, in words: PK u, v; PK' u, v; compress(PK); compress(PK'); usable
enum : uint32_t { SF_KEY_PK = 0, SF_KEY_PKP = 16, SF_KEY_WIRE = 32, SF_KEY_USABLE = 48, SF_KEY_WORDS = 64 };

// four points in affine form with one inversion between them (Z is never zero: the addition law is complete)
JJS_HD void sf_four_affine(const ext_pt& a, const ext_pt& b, const ext_pt& c, const ext_pt& d, affine_words& A, affine_words& B,
                           affine_words& C, affine_words& D) {
    const fe_n ab = fq_mul(a.z, b.z), cd = fq_mul(c.z, d.z);
    const fe_n inv = fq_inverse(fq_mul(ab, cd));
    const fe_n iab = fq_mul(inv, cd), icd = fq_mul(inv, ab);
    const fe_n ai = fq_mul(iab, b.z), bi = fq_mul(iab, a.z), ci = fq_mul(icd, d.z), di = fq_mul(icd, c.z);
    A.u = fq_to_words(fq_mul(a.x, ai)); A.v = fq_to_words(fq_mul(a.y, ai));
    B.u = fq_to_words(fq_mul(b.x, bi)); B.v = fq_to_words(fq_mul(b.y, bi));
    C.u = fq_to_words(fq_mul(c.x, ci)); C.v = fq_to_words(fq_mul(c.y, ci));
    D.u = fq_to_words(fq_mul(d.x, di)); D.v = fq_to_words(fq_mul(d.y, di));
}
// sk * G (and sk * G'), one inversion
template <bool DOUBLE>
JJS_HD void sf_derive(const sign_fixed_params& P, const words8& sk, affine_words& PK, affine_words& PKp) {
    if (DOUBLE) svg_two_affine(comb_mul(P.comb_g, sk), comb_mul(P.comb_gn, sk), PK, PKp);
    else PK = to_affine_words(comb_mul(P.comb_g, sk));
}
// the rows of a key and of a signature, each output on its own; and the zero bytes of a refusal
template <bool DOUBLE>
JJS_HD void sf_store_key(const sign_fixed_params& P, uint64_t row, const affine_words& PK, const affine_words& PKp) {
    if (P.PK_out) store_point(P.PK_out, row, PK);
    if (DOUBLE && P.PKp_out) store_point(P.PKp_out, row, PKp);
    if (P.pk_w) {
        store_words(P.pk_w, (DOUBLE ? 2 : 1) * row, compress_point(PK.u, PK.v));
        if (DOUBLE) store_words(P.pk_w, 2 * row + 1, compress_point(PKp.u, PKp.v));
    }
}
template <bool DOUBLE>
JJS_HD void sf_zero_key(const sign_fixed_params& P, uint64_t row) {
    if (P.PK_out) svg_store_zero_point(P.PK_out, row);
    if (DOUBLE && P.PKp_out) svg_store_zero_point(P.PKp_out, row);
    if (P.pk_w) {
        store_words(P.pk_w, (DOUBLE ? 2 : 1) * row, words_zero());
        if (DOUBLE) store_words(P.pk_w, 2 * row + 1, words_zero());
    }
}
template <bool DOUBLE>
JJS_HD void sf_store_sig(const sign_fixed_params& P, uint64_t row, const words8& u, const affine_words& R, const affine_words& Rp) {
    if (P.u_out) store_words(P.u_out, row, u);
    if (P.R_out) store_point(P.R_out, row, R);
    if (DOUBLE && P.Rp_out) store_point(P.Rp_out, row, Rp);
    if (P.sig_w) {
        store_words(P.sig_w, (DOUBLE ? 3 : 2) * row, u);
        store_words(P.sig_w, (DOUBLE ? 3 : 2) * row + 1, compress_point(R.u, R.v));
        if (DOUBLE) store_words(P.sig_w, 3 * row + 2, compress_point(Rp.u, Rp.v));
    }
}
template <bool DOUBLE>
JJS_HD void sf_zero_sig(const sign_fixed_params& P, uint64_t row) {
    if (P.u_out) store_words(P.u_out, row, words_zero());
    if (P.R_out) svg_store_zero_point(P.R_out, row);
    if (DOUBLE && P.Rp_out) svg_store_zero_point(P.Rp_out, row);
    if (P.sig_w)
        for (uint64_t k = 0; k < (DOUBLE ? 3u : 2u); ++k) store_words(P.sig_w, (DOUBLE ? 3 : 2) * row + k, words_zero());
}

// The keyed route's pre-pass, one lane: the key of the call into the record P.key and into the key rows.  NOT constant time.
template <bool DOUBLE>
JJS_HD void sign_fixed_key(const sign_fixed_params& P) {
    const fe_src s_sk{P.sk, 32, 0};
    const words8 sk = load_words(s_sk, 0);
    const bool ok = words_lt(sk, JJS_FR_WORDS);
    affine_words PK, PKp;
    PK.u = PK.v = PKp.u = PKp.v = words_zero();
    if (ok) sf_derive<DOUBLE>(P, sk, PK, PKp);
    uint8_t* rec = reinterpret_cast<uint8_t*>(P.key);
    store_point(rec, SF_KEY_PK / 16, PK); store_point(rec, SF_KEY_PKP / 16, PKp);
    store_words(rec, SF_KEY_WIRE / 8, compress_point(PK.u, PK.v)); store_words(rec, SF_KEY_WIRE / 8 + 1, compress_point(PKp.u, PKp.v));
    words8 flag = words_zero();
    flag.w[0] = ok ? 1u : 0u;
    store_words(rec, SF_KEY_USABLE / 8, flag);
    if (ok) sf_store_key<DOUBLE>(P, 0, PK, PKp); else sf_zero_key<DOUBLE>(P, 0);
}

// SecretKey::sign (DOUBLE: sign_double) given the RNG draw.  KEYED: the key's points come from the record of sign_fixed_key, which
// also wrote the key rows.  NOT constant time.
template <bool DOUBLE, bool KEYED>
JJS_HD void sign_fixed_item(const sign_fixed_params& P, uint64_t item, uint32_t* ws) {
    uint32_t* area = ws + TABLE_WORDS;     // transcript staging, where sign_item has it
    const fe_src s_sk{P.sk, P.sk_stride, 0}, s_rnd{P.rnd, 32, 0}, s_m{P.m, 32, 0};
    const bool shared = P.sk_stride == 0;
    const words8 sk = load_words(s_sk, item), rnd = load_words(s_rnd, item), m = load_words(s_m, item);
    const fe_src s_key{reinterpret_cast<const uint8_t*>(P.key), 0, 0};
    const bool key_ok = KEYED ? load_words(s_key, 0, SF_KEY_USABLE * 4).w[0] != 0 : words_lt(sk, JJS_FR_WORDS);
    const bool ok = key_ok && words_lt(rnd, JJS_FR_WORDS) && words_lt(m, JJS_Q_WORDS);
    P.status[item] = (uint8_t)(ok ? (uint32_t)ST_OK : (uint32_t)ST_MALFORMED);
    const bool key_rows = shared ? (!KEYED && item == 0) : !KEYED;      // this lane writes key rows, at `item`
    affine_words R, Rp, PK, PKp;
    if (!ok) {
        sf_zero_sig<DOUBLE>(P, item);
        if (!shared) sf_zero_key<DOUBLE>(P, item);                      // the item's own row (KEYED: a call of one item, behind the pre-pass)
        else if (key_rows) {                                            // the call's row: the key's, whatever this item's rnd and m are
            if (key_ok) { sf_derive<DOUBLE>(P, sk, PK, PKp); sf_store_key<DOUBLE>(P, 0, PK, PKp); }
            else sf_zero_key<DOUBLE>(P, 0);
        }
        return;
    }
    stage(area, 0, rnd); stage(area, 1, sk); stage(area, 2, small_words(DOUBLE ? 2u : 1u)); stage(area, 3, m);
    const words8 r = staged_digest(area, 4);
    if (KEYED) {
        PK.u = load_words(s_key, 0, SF_KEY_PK * 4); PK.v = load_words(s_key, 0, SF_KEY_PK * 4 + 32);
        if (DOUBLE) {
            PKp.u = load_words(s_key, 0, SF_KEY_PKP * 4); PKp.v = load_words(s_key, 0, SF_KEY_PKP * 4 + 32);
            svg_two_affine(comb_mul(P.comb_g, r), comb_mul(P.comb_gn, r), R, Rp);
        } else R = to_affine_words(comb_mul(P.comb_g, r));
    } else if (DOUBLE) {
        const ext_pt a = comb_mul(P.comb_g, r), b = comb_mul(P.comb_gn, r), c = comb_mul(P.comb_g, sk);
        sf_four_affine(a, b, c, comb_mul(P.comb_gn, sk), R, Rp, PK, PKp);
    } else {
        const ext_pt a = comb_mul(P.comb_g, r);
        svg_two_affine(a, comb_mul(P.comb_g, sk), R, PK);
    }
    words8 c;
    if (DOUBLE) {
        words8 tag;
#pragma unroll
        for (int i = 0; i < 8; ++i) tag.w[i] = JJS_DOUBLE_TAG_WORDS[i];
        stage(area, 0, tag);
        stage(area, 1, R.u); stage(area, 2, R.v); stage(area, 3, Rp.u); stage(area, 4, Rp.v);
        stage(area, 5, PK.u); stage(area, 6, PK.v); stage(area, 7, PKp.u); stage(area, 8, PKp.v); stage(area, 9, m);
        c = staged_digest(area, 10);
    } else {
        stage(area, 0, R.u); stage(area, 1, R.v); stage(area, 2, PK.u); stage(area, 3, PK.v); stage(area, 4, m);
        c = staged_digest(area, 5);
    }
    sf_store_sig<DOUBLE>(P, item, fr_sub_mul(r, c, sk), R, Rp);
    if (key_rows) sf_store_key<DOUBLE>(P, item, PK, PKp);
}

// PublicKey::from / PublicKeyDouble::from alone: the range test on sk, the comb(s) with one shared inversion, the affine and the
// wire rows and the status.  rnd, m and the signature outputs are not touched.  NOT constant time.
template <bool DOUBLE>
JJS_HD void derive_fixed_item(const sign_fixed_params& P, uint64_t item) {
    const fe_src s_sk{P.sk, 32, 0};
    const words8 sk = load_words(s_sk, item);
    const bool ok = words_lt(sk, JJS_FR_WORDS);
    P.status[item] = (uint8_t)(ok ? (uint32_t)ST_OK : (uint32_t)ST_MALFORMED);
    if (!ok) { sf_zero_key<DOUBLE>(P, item); return; }
    affine_words PK, PKp;
    sf_derive<DOUBLE>(P, sk, PK, PKp);
    sf_store_key<DOUBLE>(P, item, PK, PKp);
}

}  // namespace jjs

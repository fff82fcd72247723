// Poseidon digests of ragged inputs (include/jjs_gpu.h jjs_digest / jjs_digest_dev): item i of a call is a run of
// len(i) >= 1 field elements of one column, and its digest is dusk-poseidon's `Hash::digest(Domain::Other, &item)[0]` -- the `m`
// of every verify, sign and multisig call -- or, under the flag, `digest_truncated` (the low 250 bits).  The sponge is the one of
// hades29.h (rate-4 blocks, one call site of the permutation, the last permutation by the digest_only exit where one lane has
// the item), over a length that takes the 31 bits the SAFE tag encodes.
//
// Elements arrive in one of two formats:
//   canonical  32 bytes little endian, a value < q; a value >= q makes the ITEM malformed (status 3, a zero row), as a
//              non-canonical coordinate does in points_check.h -- the lane hashes on (straight-line arithmetic, defined on any
//              256-bit value) and its answer is discarded;
//   wide       64 bytes little endian reduced mod q: `BlsScalar::from_bytes_wide`.  Never malformed.
// Bound-tracked types of an element on its way into Montgomery form (fq29.h: fe<L, A> has limbs < L 2^29 and a value < A q):
//   a 256-bit value cut into 29-bit limbs is fe<1, 3>: the top limb has 24 bits, and 2^256 < 2.21 q;
//   canonical  fq_mul(fe<1, 3>, R'^2 <1, 1>)                                  -> fe<1, 2> = x R'            one product
//   wide       fq_mul(hi <1, 3>, JJS_TWO256 <1, 1>) = hi 2^256 mod q          -> fe<1, 2>, a plain value    the extra product
//              fq_add(lo <1, 3>, that)                                         -> fe<2, 5>
//              fq_norm                                                         -> fe<1, 5> (< 5 q < 2^258: the top limb holds it)
//              fq_mul(fe<1, 5>, R'^2 <1, 1>)                                   -> fe<1, 2> = (lo + 2^256 hi) R'
//
// Two routes run these functions (device_kernels.h): digest_kernel, one lane per item, and digest_coop_kernel, eight adjacent lanes
// per item with hades_permute(st, coop) as small_batch.h runs it -- every lane of the eight fetches the same elements, so they
// agree on the status without an exchange, and lane 0 writes.  A wave runs as long as its longest lane: a ragged call gives
// lane j item order[j], the items sorted by their count of sponge blocks, descending and stable (dg_block_order, on the host from
// the host offsets); a uniform call has neither offsets nor an order on the device.
//
// All of it is JJS_HD: tests/hostbuild/digest_harness.cpp runs these functions on the CPU.
#pragma once
#include <cstddef>
#include "hades29.h"
#include "safe_tag.h"
#include "verify_core.h"

namespace jjs {

enum : uint32_t { DG_CANONICAL = 0, DG_WIDE = 1 };
constexpr uint32_t DG_FLAG_TRUNCATED = 1u;
constexpr uint32_t DG_MAX_LEN = 0x7fffffffu;          // the tag encodes 0x80000000 | len
constexpr uint32_t DG_TABLE_TAGS = 1028;              // rows of JJS_SPONGE_TAG_LONG (lengths 0 .. 1027); beyond: dg_tag_item
constexpr int DG_COOP_LANES = 8;

struct digest_params {
    const uint8_t* in;         // the elements of every item, back to back: 32 (canonical) or 64 (wide) bytes each
    const uint32_t* offsets;   // ragged: n + 1 words, item i = elements [offsets[i], offsets[i + 1]); null: uniform
    const uint32_t* order;     // ragged: n words, the item of lane j (dg_block_order); null: lane j takes item j
    const uint32_t* tags;      // [DG_TABLE_TAGS][9]: the SAFE tags of the short lengths, Montgomery limbs
    uint32_t* long_tags;       // the tags of the lengths beyond the table, written by dg_tag_item: 9 words per item of a ragged call
    uint32_t long_stride;      // ... (long_stride = 9), one tag for a uniform call (0); null when no item is that long
    uint8_t* out;              // n x 32
    uint8_t* status;           // nullable, n bytes
    uint64_t n;
    uint32_t k;                // uniform: the length of every item
    uint32_t flags;            // DG_FLAG_TRUNCATED
};

JJS_HD uint32_t dg_blocks(uint32_t len) { return (len >> 2) + ((len & 3u) ? 1u : 0u); }

// The order of a ragged call: the items by dg_blocks(len), descending, equal counts in input order.  A counting sort on the
// count, one byte of it at a time from the lowest (each pass stable, so the whole is) and only over the bytes in which two items
// differ: one pass for items of fewer than 1 024 elements.  `order` and `tmp` are n words each; the answer is in `order`.  Plain
// C++, run by the entry point on the host offsets; it allocates nothing.
inline void dg_block_order(const uint32_t* offsets, size_t n, uint32_t* tmp, uint32_t* order) {
    uint32_t differ = 0;
    const uint32_t c0 = n ? dg_blocks(offsets[1] - offsets[0]) : 0u;
    for (size_t i = 0; i < n; ++i) {
        order[i] = (uint32_t)i;
        differ |= dg_blocks(offsets[i + 1] - offsets[i]) ^ c0;
    }
    uint32_t *src = order, *dst = tmp;
    for (int shift = 0; shift < 32; shift += 8) {
        if (!((differ >> shift) & 0xffu)) continue;
        size_t place[257] = {};
        auto digit = [&](uint32_t item) { return 255u - ((dg_blocks(offsets[item + 1] - offsets[item]) >> shift) & 0xffu); };   // descending
        for (size_t i = 0; i < n; ++i) ++place[digit(src[i]) + 1];
        for (int d = 0; d < 256; ++d) place[d + 1] += place[d];
        for (size_t i = 0; i < n; ++i) dst[place[digit(src[i])]++] = src[i];
        uint32_t* t = src; src = dst; dst = t;
    }
    if (src != order)
        for (size_t i = 0; i < n; ++i) order[i] = src[i];
}

JJS_HD fe<1, 3> dg_limbs(const words8& w) { return fq_as<1, 3>(words_to_limbs(w)); }

// element e of the run at `p` in Montgomery form; canonical: `bad` is raised when it is >= q
template <uint32_t FMT>
JJS_HD fe_n dg_element(const uint8_t* p, uint32_t e, bool& bad) {
    if (FMT == DG_WIDE) {
        const fe_src s{p, 64, 0};
        const words8 lo = load_words(s, e), hi = load_words(s, e, 32);
        const fe_n top = fq_mul(dg_limbs(hi), fe_from_const<1, 1>(JJS_TWO256));          // hi 2^256 mod q, a plain value
        return fq_mul(fq_norm(fq_add(dg_limbs(lo), top)), fe_from_const<1, 1>(JJS_R2));
    }
    const fe_src s{p, 32, 0};
    const words8 w = load_words(s, e);
    bad = bad || !words_lt(w, JJS_Q_WORDS);
    return fq_mul(dg_limbs(w), fe_from_const<1, 1>(JJS_R2));
}

// where the item of lane / group `j` lies: its index (a call has fewer than 2^32 items), its length, its first element
struct dg_item { uint32_t item, len; const uint8_t* p; };
template <uint32_t FMT>
JJS_HD dg_item dg_locate(const digest_params& D, uint64_t j) {
    dg_item it;
    it.item = D.order ? D.order[j] : (uint32_t)j;
    uint64_t first;
    if (D.offsets) { first = D.offsets[it.item]; it.len = D.offsets[it.item + 1] - D.offsets[it.item]; }
    else { first = (uint64_t)it.item * D.k; it.len = D.k; }
    it.p = D.in + first * (FMT == DG_WIDE ? 64u : 32u);
    return it;
}

// The SAFE tag of a `len`-element absorb comes from the table, or, beyond it, from a pass in front (one lane per item of a ragged
// call, one lane for a uniform call; as pass 0 of the multisig kernels): BLAKE2b and 773 doublings mod q once per item, in a
// kernel of their own so that the lanes that hash keep the registers of the hash alone.
JJS_HD void dg_tag_item(const digest_params& D, uint64_t item) {
    const uint32_t len = D.offsets ? D.offsets[item + 1] - D.offsets[item] : D.k;
    if (len < DG_TABLE_TAGS) return;
    uint32_t q[8], limbs[9];
    for (int i = 0; i < 8; ++i) q[i] = JJS_Q_WORDS[i];
    safe_tag_limbs(len, q, limbs);
    for (int i = 0; i < 9; ++i) D.long_tags[(size_t)D.long_stride * item + i] = limbs[i];
}
JJS_HD fe_n dg_tag(const digest_params& D, uint64_t item, uint32_t len) {
    const uint32_t* src = len < DG_TABLE_TAGS ? D.tags + (size_t)len * 9 : D.long_tags + (size_t)D.long_stride * item;
    fe_n t;
#pragma unroll
    for (int i = 0; i < 9; ++i) t.l[i] = src[i];
    return t;
}

// poseidon_digest_tagged of hades29.h over the `len` elements at p, len in [1, 2^31 - 1]: rate-4 blocks and one call site of the
// permutation as there, but the sponge walks -- a pointer to the block and the count of elements left are all that lives across a
// permutation, and no block count is formed (there: (len + 3) >> 2 in an int).  An item ends with a permutation (len >= 1), by the
// digest_only exit when one lane has it.
template <uint32_t FMT>
JJS_HD fe_n dg_sponge(const uint8_t* p, uint32_t len, const fe_n& tag, bool& bad, int coop) {
    hades_state st;
    st.s[0] = tag;
#pragma unroll
    for (int i = 1; i < 5; ++i) st.s[i] = fq_as<1, 2>(fq_zero());
    for (uint32_t left = len;; left -= 4, p += 4 * (FMT == DG_WIDE ? 64 : 32)) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (k < left) st.s[1 + k] = fq_reduce(fq_norm(fq_add(st.s[1 + k], dg_element<FMT>(p, k, bad))));
        const bool last = left <= 4;
        hades_permute(st, coop, coop < 0 && last);
        if (last) break;
    }
    return st.s[1];
}

// The item of lane `j` (lane route: coop < 0), or of the eight lanes of which this is lane `coop`: the digest, and when `write` is
// set (lane 0 of the eight, every lane of the lane route) the row and the status byte.
template <uint32_t FMT>
JJS_HD void dg_lane(const digest_params& D, uint64_t j, int coop, bool write) {
    const dg_item it = dg_locate<FMT>(D, j);
    bool bad = false;
    const fe_n d = dg_sponge<FMT>(it.p, it.len, dg_tag(D, it.item, it.len), bad, coop);
    words8 w = (D.flags & DG_FLAG_TRUNCATED) ? truncate250(d) : fq_to_words(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) w.w[i] = bad ? 0u : w.w[i];
    if (!write) return;
    store_words(D.out, it.item, w);
    if (D.status) D.status[it.item] = bad ? (uint8_t)ST_MALFORMED : (uint8_t)ST_OK;
}

}  // namespace jjs

// CPU build of csrc/digest.h (Poseidon digests of ragged inputs) for tests/test_digest_host.py: the JJS_HD functions of the
// device's one-lane-per-item route -- dg_tag_item in front, dg_lane over dg_locate, dg_tag, dg_sponge, dg_element -- one item after the other on this
// thread, in the order dg_block_order gives a ragged call or in input order; and the pieces on their own.  The eight-lane route
// exists on the device only.
#include "host_harness.cpp"
#include "digest.h"

extern "C" {

// the arguments of jjs_digest, every buffer 16-byte aligned; ordered != 0: a ragged call's lanes take the items by dg_block_order
int jjs_dg_host_digest(int format, int flags, const uint8_t* in, const uint32_t* offsets, size_t k, size_t n, uint8_t* out, uint8_t* status,
                       int ordered) {
    if ((format != (int)DG_CANONICAL && format != (int)DG_WIDE) || (flags & ~(int)DG_FLAG_TRUNCATED)) return -1;
    std::vector<uint32_t> order(2 * n + 1);
    digest_params D{};
    D.in = in; D.offsets = offsets; D.out = out; D.status = status; D.n = n; D.k = (uint32_t)k; D.flags = (uint32_t)flags;
    D.tags = &JJS_SPONGE_TAG_LONG[0][0];
    if (offsets && ordered) {
        dg_block_order(offsets, n, order.data() + n, order.data());
        D.order = order.data();
    }
    std::vector<uint32_t> long_tags(9 * n + 9);
    D.long_tags = long_tags.data(); D.long_stride = offsets ? 9u : 0u;
    for (uint64_t i = 0; i < (offsets ? n : 1); ++i) dg_tag_item(D, i);        // the pass in front
    for (uint64_t j = 0; j < n; ++j) {
        if (format == (int)DG_WIDE) dg_lane<DG_WIDE>(D, j, -1, true);
        else dg_lane<DG_CANONICAL>(D, j, -1, true);
    }
    return 0;
}
void jjs_dg_host_order(const uint32_t* offsets, size_t n, uint32_t* order) {
    std::vector<uint32_t> tmp(n + 1);
    dg_block_order(offsets, n, tmp.data(), order);
}
// one element into Montgomery form and back: 32 canonical bytes out; returns the range test's finding
int jjs_dg_host_element(int format, const uint8_t* in, uint8_t* out) {
    bool bad = false;
    const fe_n x = format == (int)DG_WIDE ? dg_element<DG_WIDE>(in, 0, bad) : dg_element<DG_CANONICAL>(in, 0, bad);
    const words8 w = fq_to_words(x);
    memcpy(out, w.w, 32);
    return bad ? 1 : 0;
}
// the tag of a len-element absorb as the lanes get it (a uniform call of that length), canonical bytes
void jjs_dg_host_tag(uint32_t len, uint8_t* out) {
    uint32_t slot[9] = {};
    digest_params D{};
    D.tags = &JJS_SPONGE_TAG_LONG[0][0]; D.long_tags = slot; D.k = len; D.n = 1;
    dg_tag_item(D, 0);
    const words8 w = fq_to_words(dg_tag(D, 0, len));
    memcpy(out, w.w, 32);
}
uint32_t jjs_dg_host_blocks(uint32_t len) { return dg_blocks(len); }
void jjs_dg_host_two256(uint8_t* out) {
    const words8 w = fq_to_words(fq_as<1, 2>(fe_from_const<1, 1>(JJS_TWO256)));
    memcpy(out, w.w, 32);
}

}  // extern "C"

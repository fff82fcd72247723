// CPU build of csrc/msig_scratch.h (the layout and the growth of the device's multisignature scratch) for
// tests/test_msig_scratch_host.py: the walk over the regions at a base address the test chooses, and the growth rule.
#include "msig_scratch.h"

using namespace jjs;

static msig_caps caps_of(const uint64_t v[9]) {
    msig_caps c;
    for (int i = 0; i < 9; ++i) c.*MSIG_DIMS[i].cap = (size_t)v[i];
    return c;
}

extern "C" {

int jjs_msig_scratch_ext_words(void) { return EXT_WORDS; }

// caps[9]: rows, transcripts, ext rows, key-set rows and transcripts, sign rows and transcripts, share queries and transcripts.
// regions[24]: the address of every region in the order of tests/msig_scratch_hostlib.py REGIONS (0: null).  Returns the bytes.
uint64_t jjs_msig_scratch_layout(uint64_t base, const uint64_t caps[9], uint64_t regions[24], uint64_t* sign_flag_words) {
    const msig_layout Y = msig_scratch_layout(reinterpret_cast<uint8_t*>((uintptr_t)base), caps_of(caps));
    const msig_scratch& W = Y.W;
    const void* const r[24] = {W.tr_of, W.d_words, W.dpk, W.e_pt, W.a_words, W.c_words, W.offsets, W.long_tags, W.norm[0], W.norm[1], W.norm[2], W.prefix,
                               W.ks_pk, W.ks_row_key, W.ks_refused, W.pk_repeats, W.bad_enc, W.dup_nonce, W.sign_agg, W.sign_rsa,
                               W.share_pt, W.share_bad, W.share_agg, W.share_rsa};
    for (int i = 0; i < 24; ++i) regions[i] = (uint64_t)reinterpret_cast<uintptr_t>(r[i]);
    *sign_flag_words = W.sign_flag_words;
    return Y.bytes;
}

void jjs_msig_scratch_grown(const uint64_t held[9], const uint64_t need[9], uint64_t out[9]) {
    const msig_caps c = msig_caps_grown(caps_of(held), caps_of(need));
    for (int i = 0; i < 9; ++i) out[i] = c.*MSIG_DIMS[i].cap;
}

}  // extern "C"

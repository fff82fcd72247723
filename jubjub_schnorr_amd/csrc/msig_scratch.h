// The device's multisignature scratch (device_state::msig): its capacities, how they grow, and where its regions lie.  Plain C++
// without HIP or engine state: tests/hostbuild/msig_scratch_harness.cpp compiles it for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "grown.h"
#include "multisig_core.h"

namespace jjs {

// What the scratch holds room for.  rows and transcripts: every call.  The others are 0 until a call asks for them, and no other
// caller pays for them: ext_rows an *_ext or *_wire call, ks_* a key-set call (msig_keyset.h), sign_* a signing call (msig_sign.h),
// share_* a verify_share call (msig_share.h; there may be more queries than rows).
struct msig_caps {
    size_t rows = 0, transcripts = 0;
    size_t ext_rows = 0;
    size_t ks_rows = 0, ks_transcripts = 0;
    size_t sign_rows = 0, sign_transcripts = 0;
    size_t share_queries = 0, share_transcripts = 0;
};

// A dimension never holds less than `floor` once it holds anything, and an optional one grows only when `asked_by` is asked for:
// the transcripts of an optional region follow its rows.
struct msig_dim { size_t msig_caps::*cap; size_t floor; size_t msig_caps::*asked_by; };
constexpr msig_dim MSIG_DIMS[9] = {
    {&msig_caps::rows, 4096, nullptr},
    {&msig_caps::transcripts, 1024, nullptr},
    {&msig_caps::ext_rows, 4096, &msig_caps::ext_rows},
    {&msig_caps::ks_rows, 4096, &msig_caps::ks_rows},
    {&msig_caps::ks_transcripts, 1024, &msig_caps::ks_rows},
    {&msig_caps::sign_rows, 4096, &msig_caps::sign_rows},
    {&msig_caps::sign_transcripts, 1024, &msig_caps::sign_rows},
    {&msig_caps::share_queries, 4096, &msig_caps::share_queries},
    {&msig_caps::share_transcripts, 1024, &msig_caps::share_queries},
};

inline bool operator==(const msig_caps& a, const msig_caps& b) {
    for (const msig_dim& d : MSIG_DIMS)
        if (a.*d.cap != b.*d.cap) return false;
    return true;
}
// The capacities after a call that needs `need` of a scratch that holds `held`: `held` itself when it suffices (nothing is
// allocated then), else every dimension anew -- never below what is held, and an optional one nobody has asked for stays 0.
inline msig_caps msig_caps_grown(const msig_caps& held, const msig_caps& need) {
    bool fits = true;
    for (const msig_dim& d : MSIG_DIMS) fits = fits && need.*d.cap <= held.*d.cap;
    if (fits) return held;
    msig_caps c;
    for (const msig_dim& d : MSIG_DIMS) {
        const size_t want = need.*d.cap < d.floor ? d.floor : need.*d.cap;
        const size_t cap = !d.asked_by || need.*d.asked_by ? grown(want) : 0;
        c.*d.cap = cap < held.*d.cap ? held.*d.cap : cap;
    }
    return c;
}

// The regions.  Point and scalar columns that kernels or build_call read sixteen bytes at a time are 64-byte aligned, word
// regions 4-byte aligned; the region of a dimension that is 0 is null.
struct msig_scratch {
    uint32_t *tr_of, *d_words, *dpk, *e_pt;      // per row: 1, 8, EXT_WORDS, EXT_WORDS words
    uint32_t *a_words, *c_words, *long_tags;     // per transcript: 8, 8, 18 words
    uint32_t* offsets;                           // transcripts + 1 words
    uint8_t* norm[3];                            // ext: three columns of normalised or decoded points, 64 bytes per row each
    uint32_t* prefix;                            // ext: the 9 words of prefix product per row that normalize_lane keeps
    uint8_t* ks_pk;                              // key set: the gathered key column, 64 bytes per row
    uint32_t *ks_row_key, *ks_refused;           // key set: the table index of every row, the refused word of every transcript
    uint32_t *pk_repeats, *bad_enc, *dup_nonce;  // sign: the check pass's flag words, [rows], [transcripts], [transcripts] -- one
    size_t sign_flag_words;                      // run of this many words from pk_repeats, which the call clears with one memset
    uint8_t *sign_agg, *sign_rsa;                // sign: pk_agg and RSa, which a signing call has no output for, 64 bytes per transcript
    uint32_t *share_pt, *share_bad;              // share: [queries][EXT_WORDS], [transcripts]
    uint8_t *share_agg, *share_rsa;              // share: pk_agg and RSa, which such a call may have no output for, 64 bytes per transcript
};
struct msig_layout {
    msig_scratch W;
    size_t bytes;
};

// The one walk over the regions of a scratch of capacities c at `base` (64-byte aligned; null: only the size is wanted).  The byte
// count is where the walk ends.
inline msig_layout msig_scratch_layout(uint8_t* base, const msig_caps& c) {
    msig_scratch W{};
    size_t at = 0;
    auto words = [&](uint32_t*& region, size_t count) {
        region = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(base) + at);
        at += 4 * count;
    };
    auto column = [&](uint8_t*& region, size_t rows) {
        at = (at + 63) & ~size_t(63);
        region = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(base) + at);
        at += 64 * rows;
    };
    words(W.tr_of, c.rows);
    words(W.d_words, 8 * c.rows);
    words(W.dpk, EXT_WORDS * c.rows);
    words(W.e_pt, EXT_WORDS * c.rows);
    words(W.a_words, 8 * c.transcripts);
    words(W.c_words, 8 * c.transcripts);
    words(W.long_tags, 18 * c.transcripts);
    words(W.offsets, c.transcripts + 1);
    if (c.ext_rows) {
        for (uint8_t*& col : W.norm) column(col, c.ext_rows);
        words(W.prefix, 9 * c.ext_rows);
    }
    if (c.ks_rows) {
        column(W.ks_pk, c.ks_rows);
        words(W.ks_row_key, c.ks_rows);
        words(W.ks_refused, c.ks_transcripts);
    }
    if (c.sign_rows) {
        column(W.sign_agg, c.sign_transcripts);
        column(W.sign_rsa, c.sign_transcripts);
        words(W.pk_repeats, c.sign_rows);
        words(W.bad_enc, c.sign_transcripts);
        words(W.dup_nonce, c.sign_transcripts);
        W.sign_flag_words = c.sign_rows + 2 * c.sign_transcripts;
    }
    if (c.share_queries) {
        column(W.share_agg, c.share_transcripts);
        column(W.share_rsa, c.share_transcripts);
        words(W.share_pt, EXT_WORDS * c.share_queries);
        words(W.share_bad, c.share_transcripts);
    }
    return msig_layout{W, at};
}

}  // namespace jjs

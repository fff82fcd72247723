// The bucket method of csrc/msm.h on the CPU, for verdict_harness.cpp and keyset_verdict_harness.cpp (included after
// host_harness.cpp): the device's steps in loops -- the counting sort of the terms, one bucket, one segment and one window at
// a time, Horner's rule -- with the same functions.
#pragma once
#include "msm.h"

namespace {

// sum of the terms (terms: N cached addends; scalars N x 32) by the bucket method of shape S; neg(t): term t is a negated point
template <class Neg>
ext_pt host_msm(const uint32_t* terms, const uint8_t* scalars, uint64_t N, const msm_shape& S, Neg neg) {
    std::vector<uint32_t> off((size_t)S.W * S.B + 1, 0), order;
    for (int pass = 0; pass < 2; ++pass) {                     // 0: count, 1: scatter
        std::vector<uint32_t> cursor;
        if (pass) {
            uint32_t sum = 0;
            for (size_t i = 0; i < off.size(); ++i) { const uint32_t v = off[i]; off[i] = sum; sum += v; }
            order.assign(sum, 0);
            cursor.assign(off.begin(), off.end());
        }
        for (uint64_t t = 0; t < N; ++t) {
            const words8 s = load_words(fe_src{scalars, 32, 0}, t);
            uint32_t carry = 0;
            for (int j = 0; j < S.W; ++j) {
                const int32_t d = msm_digit_step(s, j, S.c, S.W, carry);
                if (!d) continue;
                const uint32_t slot = msm_slot_split(j, d, t, S.W, S.top_split);
                if (slot >= S.B) continue;             // (never: scalars within the shape's bits keep every digit in range)
                const uint32_t id = (uint32_t)j * S.B + slot;
                if (!pass) ++off[id];
                else order[cursor[id]++] = (uint32_t)t | (((d < 0) != neg(t)) ? MSM_NEG : 0u);
            }
        }
    }
    std::vector<uint32_t> buckets((size_t)S.W * S.B * MSM_EXT_WORDS), win((size_t)S.W * MSM_EXT_WORDS);
    for (uint32_t id = 0; id < (uint32_t)S.W * S.B; ++id) msm_store_ext(&buckets[(size_t)id * MSM_EXT_WORDS], msm_bucket(off.data(), order.data(), terms, id));
    for (int j = 0; j < S.W; ++j) {
        ext_pt acc = ext_identity();
        for (uint32_t seg = 0; seg < S.K; ++seg) acc = msm_add_ext(acc, msm_segment(buckets.data(), S.B, (uint32_t)j, seg, S.L, j == S.W - 1 ? S.top_split : 0));
        msm_store_ext(&win[(size_t)j * MSM_EXT_WORDS], acc);
    }
    return msm_combine(win.data(), S.W, S.c);
}

template <class T>
T* align16(std::vector<T>& v) { return (T*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); }

void to_affine_bytes(const ext_pt& p, uint8_t* out) {
    const fe_n zi = fq_inverse(p.z);
    store_words(out, 0, fq_to_words(fq_mul(p.x, zi)));
    store_words(out, 1, fq_to_words(fq_mul(p.y, zi)));
}

}  // namespace

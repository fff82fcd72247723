// The bucket method of csrc/msm.h on the CPU, for verdict_harness.cpp and keyset_verdict_harness.cpp (included after
// host_harness.cpp): the device's steps in loops -- the counting sort of the terms, one bucket, one segment and one window at
// a time, Horner's rule -- with the same functions.
#pragma once
#include <thread>
#include "msm.h"

namespace {

// fn(i) for i in [0, n) on up to eight threads (the units are independent, as the device's lanes are): a wide window has
// 2^19 buckets, whose segments cost a second or more on one core whatever the number of terms
template <class Fn>
void host_parallel_for(size_t n, Fn fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t workers = n < 4096 ? 1 : (hw < 1 ? 1 : (hw > 8 ? 8 : hw));
    if (workers == 1) { for (size_t i = 0; i < n; ++i) fn(i); return; }
    std::vector<std::thread> pool;
    for (size_t w = 0; w < workers; ++w)
        pool.emplace_back([=] { for (size_t i = n * w / workers; i < n * (w + 1) / workers; ++i) fn(i); });
    for (std::thread& t : pool) t.join();
}

// what the stages of host_msm leave, for a caller that wants them: the buckets' offsets (W * B + 1), the sorted entries, the
// window sums (W extended points)
struct host_msm_stages {
    std::vector<uint32_t> off, order, win;
};
// sum of the terms (terms: N cached addends; scalars N x 32) by the bucket method of shape S; neg(t): term t is a negated point
template <class Neg>
ext_pt host_msm(const uint32_t* terms, const uint8_t* scalars, uint64_t N, const msm_shape& S, Neg neg, host_msm_stages* stages = nullptr) {
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
    std::vector<uint32_t> buckets((size_t)S.W * S.B * MSM_EXT_WORDS), segs((size_t)S.W * S.K * MSM_EXT_WORDS), win((size_t)S.W * MSM_EXT_WORDS);
    host_parallel_for((size_t)S.W * S.B, [&](size_t id) { msm_store_ext(&buckets[id * MSM_EXT_WORDS], msm_bucket(off.data(), order.data(), terms, (uint32_t)id)); });
    host_parallel_for((size_t)S.W * S.K, [&](size_t id) {
        const uint32_t j = (uint32_t)(id / S.K);
        msm_store_ext(&segs[id * MSM_EXT_WORDS], msm_segment(buckets.data(), S.B, j, (uint32_t)(id % S.K), S.L, (int)j == S.W - 1 ? S.top_split : 0));
    });
    for (int j = 0; j < S.W; ++j) {
        ext_pt acc = ext_identity();
        for (uint32_t seg = 0; seg < S.K; ++seg) acc = msm_add_ext(acc, msm_load_ext(&segs[((size_t)j * S.K + seg) * MSM_EXT_WORDS]));
        msm_store_ext(&win[(size_t)j * MSM_EXT_WORDS], acc);
    }
    const ext_pt total = msm_combine(win.data(), S.W, S.c);
    if (stages) { stages->off.swap(off); stages->order.swap(order); stages->win.swap(win); }
    return total;
}

template <class T>
T* align16(std::vector<T>& v) { return (T*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); }

void to_affine_bytes(const ext_pt& p, uint8_t* out) {
    const fe_n zi = fq_inverse(p.z);
    store_words(out, 0, fq_to_words(fq_mul(p.x, zi)));
    store_words(out, 1, fq_to_words(fq_mul(p.y, zi)));
}

}  // namespace

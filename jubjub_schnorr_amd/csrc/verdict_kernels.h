// Part of jjs_gpu.hip (included inside its anonymous namespace, after device_kernels.h): the kernels of the batch verdict
// (batch_verdict.h, msm.h; verdict_calls.h launches them).
#pragma once

// the MSM's launches: terms and scalars from bv_item_kernel, then the sort, buckets, segments and windows of msm.h
struct msm_params : msm_shape {       // c, W, top_split, B, K, L
    const uint32_t* terms;
    const uint8_t* scalars;
    uint64_t n, N;                    // items, terms (n_kinds * n)
    uint32_t neg_kinds;               // bit k: the terms of kind k are negated points
    uint32_t* off;                    // W * B + 1: counts, then their exclusive prefix sums
    uint32_t* cursor;                 // W * B: the scatter's positions
    uint32_t* order;                  // the sorted entries: term | MSM_NEG
    uint32_t* buckets;                // W * B extended points
    uint32_t* segs;                   // W * K extended points
    uint32_t* win;                    // W extended points
};

// red[0 .. MSM_EXT_WORDS) = the sum over the block's lanes of acc, by a tree (red: BLOCK * MSM_EXT_WORDS words)
__device__ inline void block_sum_ext(uint32_t* red, const ext_pt& acc) {
    msm_store_ext(red + threadIdx.x * MSM_EXT_WORDS, acc);
    __syncthreads();
    for (int step = BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step)
            msm_store_ext(red + threadIdx.x * MSM_EXT_WORDS,
                          msm_add_ext(msm_load_ext(red + threadIdx.x * MSM_EXT_WORDS), msm_load_ext(red + (threadIdx.x + step) * MSM_EXT_WORDS)));
        __syncthreads();
    }
}

// The per-item pass (item = bv_item or ksv_item on its params): one lane per item (grid-stride), the sums of z u (z' u) per
// block, a failed check clears the verdict (one atomic per wave, from the ballot).
template <class P, class Item>
__device__ inline void verdict_item_pass(const P& B, Item item_fn) {
    __shared__ words8 red[2][BLOCK];
    words8 acc[2] = {words_zero(), words_zero()};
    const uint64_t total = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t base = 0; base < B.V.n; base += total) {
        const uint64_t item = base + (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
        const bool active = item < B.V.n;
        bool ok = true;
        if (active) {
            words8 zu[2];
            ok = item_fn(B, item, zu);
            acc[0] = fr_add(acc[0], zu[0]);
            acc[1] = fr_add(acc[1], zu[1]);
        }
        if (__ballot(!ok) && (threadIdx.x & 63) == 0) atomicOr(B.fail, 1u);
    }
    red[0][threadIdx.x] = acc[0];
    red[1][threadIdx.x] = acc[1];
    __syncthreads();
    for (int step = BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step)
            for (int e = 0; e < 2; ++e) red[e][threadIdx.x] = fr_add(red[e][threadIdx.x], red[e][threadIdx.x + step]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        store_words(B.partial, 2 * blockIdx.x, red[0][0]);
        store_words(B.partial, 2 * blockIdx.x + 1, red[1][0]);
    }
}
__global__ __launch_bounds__(BLOCK, 2) void bv_item_kernel(bv_params B) {
    verdict_item_pass(B, [](const bv_params& b, uint64_t item, words8* zu) { return bv_item(b, item, zu); });
}

// counting sort of (window, |digit|): count (scatter = false), then place (scatter = true); one lane per term
template <bool scatter>
__global__ __launch_bounds__(BLOCK) void msm_sort_kernel(msm_params M) {
    const uint64_t total = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; t < M.N; t += total) {
        const words8 s = load_words(fe_src{M.scalars, 32, 0}, t);
        const bool neg = (M.neg_kinds >> (uint32_t)(t / M.n)) & 1u;
        uint32_t carry = 0;
        for (int j = 0; j < M.W; ++j) {
            const int32_t d = msm_digit_step(s, j, M.c, M.W, carry);
            if (!d) continue;
            const uint32_t slot = msm_slot_split(j, d, t, M.W, M.top_split);
            if (slot >= M.B) continue;             // (scalars below 2^252 keep every digit in range)
            const uint32_t id = (uint32_t)j * M.B + slot;
            if (!scatter) atomicAdd(&M.off[id], 1u);
            else M.order[atomicAdd(&M.cursor[id], 1u)] = (uint32_t)t | (((d < 0) != neg) ? MSM_NEG : 0u);
        }
    }
}
// exclusive prefix sums of the W * B counts, copied to the cursors: msm_scan_kernel<0> sums each block's MSM_SCAN_SPAN
// counts (one block per span), msm_scan_kernel<1> (one block) scans those sums, msm_scan_kernel<2> scans within each span
constexpr uint32_t MSM_SCAN_SPAN = 4096;
template <int phase>
__global__ __launch_bounds__(1024) void msm_scan_kernel(msm_params M, uint32_t* span_sum) {
    __shared__ uint32_t part[1024];
    const uint32_t cnt = (uint32_t)M.W * M.B, spans = (cnt + MSM_SCAN_SPAN - 1) / MSM_SCAN_SPAN;
    const uint32_t tid = threadIdx.x;
    uint32_t v[4] = {0u, 0u, 0u, 0u}, sum = 0;
    const uint32_t base = phase == 1 ? 4 * tid : blockIdx.x * MSM_SCAN_SPAN + 4 * tid;      // four entries per lane
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = base + k;
        v[k] = phase == 1 ? (i < spans ? span_sum[i] : 0u) : (i < cnt ? M.off[i] : 0u);
        sum += v[k];
    }
    part[tid] = sum;
    __syncthreads();
    for (uint32_t step = 1; step < 1024; step <<= 1) {
        const uint32_t x = tid >= step ? part[tid - step] : 0u;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    if (phase == 0) {
        if (tid == 1023) span_sum[blockIdx.x] = part[1023];
        return;
    }
    uint32_t run = part[tid] - sum + (phase == 2 ? span_sum[blockIdx.x] : 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = base + k;
        if (phase == 1) {
            if (i < spans) span_sum[i] = run;           // exclusive: the counts before span i
        } else if (i < cnt) {
            M.off[i] = run; M.cursor[i] = run;
        }
        run += v[k];
    }
    if (phase == 1 && tid == 1023) span_sum[spans] = part[1023];
    if (phase == 2 && blockIdx.x == spans - 1 && tid == 1023) M.off[cnt] = run;
}
__global__ __launch_bounds__(BLOCK, 2) void msm_bucket_kernel(msm_params M) {
    const uint32_t id = blockIdx.x * BLOCK + threadIdx.x;
    if (id >= (uint32_t)M.W * M.B) return;
    msm_store_ext(M.buckets + (size_t)id * MSM_EXT_WORDS, msm_bucket(M.off, M.order, M.terms, id));
}
__global__ __launch_bounds__(BLOCK, 2) void msm_segment_kernel(msm_params M) {
    const uint32_t id = blockIdx.x * BLOCK + threadIdx.x;
    if (id >= (uint32_t)M.W * M.K) return;
    const uint32_t j = id / M.K;
    msm_store_ext(M.segs + (size_t)id * MSM_EXT_WORDS, msm_segment(M.buckets, M.B, j, id % M.K, M.L, j + 1 == (uint32_t)M.W ? M.top_split : 0));
}
// one block per window: its K segments added
__global__ __launch_bounds__(BLOCK) void msm_window_kernel(msm_params M) {
    __shared__ uint32_t red[BLOCK * MSM_EXT_WORDS];
    const uint32_t j = blockIdx.x;
    ext_pt acc = ext_identity();
    for (uint32_t k = threadIdx.x; k < M.K; k += BLOCK) acc = msm_add_ext(acc, msm_load_ext(M.segs + ((size_t)j * M.K + k) * MSM_EXT_WORDS));
    block_sum_ext(red, acc);
    if (threadIdx.x < MSM_EXT_WORDS) M.win[(size_t)j * MSM_EXT_WORDS + threadIdx.x] = red[threadIdx.x];
}
// The blocks' partial sums of z u (z' u) added by one block: every lane takes its share of the blocks, then a tree.  Every
// lane returns with the two totals in sum[0], sum[1].
__device__ inline void verdict_sum_partials(const uint8_t* partial, uint32_t blocks, words8 sum[2]) {
    __shared__ words8 red[2][BLOCK];
    words8 acc[2] = {words_zero(), words_zero()};
    for (uint32_t b = threadIdx.x; b < blocks; b += BLOCK) {
        acc[0] = fr_add(acc[0], load_words(fe_src{partial, 32, 0}, 2 * b));
        acc[1] = fr_add(acc[1], load_words(fe_src{partial, 32, 0}, 2 * b + 1));
    }
    red[0][threadIdx.x] = acc[0];
    red[1][threadIdx.x] = acc[1];
    __syncthreads();
    for (int step = BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step)
            for (int e = 0; e < 2; ++e) red[e][threadIdx.x] = fr_add(red[e][threadIdx.x], red[e][threadIdx.x + step]);
        __syncthreads();
    }
    sum[0] = red[0][0];
    sum[1] = red[1][0];
}
// one block: the per-block sums of z u added, the windows combined, the fixed-base part, the verdict word
__global__ __launch_bounds__(BLOCK) void bv_final_kernel(bv_params B, msm_params M, uint32_t blocks, uint32_t* verdict) {
    words8 zu[2];
    verdict_sum_partials(B.partial, blocks, zu);
    if (threadIdx.x == 0) {
        const ext_pt total = msm_combine(M.win, M.W, M.c);
        *verdict = bv_verdict(B.V, total, zu, *B.fail != 0u) ? 1u : 0u;
    }
}
// the per-item route: verdict = (every item has status 0)
__global__ void tally_verdict_kernel(const unsigned long long* tally, uint64_t n, uint32_t* verdict) {
    if (threadIdx.x == 0) *verdict = tally[0] == n ? 1u : 0u;
}

#if defined(JJS_PROFILING)
// jjs_debug_msm_dev (include/jjs_gpu_profiling.h): the caller's points and scalars as an item pass leaves them, one lane per term
__global__ __launch_bounds__(BLOCK) void dbg_msm_terms_kernel(const uint8_t* points, const uint8_t* scalars, uint64_t N, uint32_t* terms,
                                                              uint8_t* term_scalars) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= N) return;
    const fe_src src{points, 64, 0};
    msm_store_term(terms + t * MSM_TERM_WORDS, load_fq(src, t), load_fq(src, t, 32));
    store_words(term_scalars, t, load_words(fe_src{scalars, 32, 0}, t));
}
// jjs_debug_verdict_items_dev, jjs_debug_keyset_items_dev: the final kernels' sum of the item pass's partial sums, written out
__global__ __launch_bounds__(BLOCK) void dbg_verdict_totals_kernel(const uint8_t* partial, uint32_t blocks, uint8_t* zu_out) {
    words8 zu[2];
    verdict_sum_partials(partial, blocks, zu);
    if (threadIdx.x == 0) {
        store_words(zu_out, 0, zu[0]);
        store_words(zu_out, 1, zu[1]);
    }
}
// ... and what the MSM left: off (W * B + 1 words), order (off[W * B] words), win (W points), msm_combine(win) from one lane
__global__ __launch_bounds__(BLOCK) void dbg_msm_out_kernel(msm_params M, uint32_t* off_out, uint32_t* order_out, uint32_t* win_out,
                                                            uint32_t* total_out) {
    const uint64_t nb = (uint64_t)M.W * M.B, total = (uint64_t)gridDim.x * BLOCK, id = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t room = M.N * (uint64_t)M.W, entries = M.off[nb] < room ? M.off[nb] : room;
    for (uint64_t i = id; i <= nb; i += total) off_out[i] = M.off[i];
    for (uint64_t i = id; i < entries; i += total) order_out[i] = M.order[i];
    for (uint64_t i = id; i < (uint64_t)M.W * MSM_EXT_WORDS; i += total) win_out[i] = M.win[i];
    if (id == 0) msm_store_ext(total_out, msm_combine(M.win, M.W, M.c));
}
#endif

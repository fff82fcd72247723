// Part of jjs_gpu.hip (included inside its anonymous namespace, after verdict_kernels.h): the kernels of the batch verdict
// against a registered key set (keyset_verdict.h; keyset_verdict_calls.h launches them, around the MSM kernels of
// verdict_kernels.h for the R terms).
#pragma once

// the run sums and the key points: the sorted items, the per-item scalar columns, the set's point columns
struct ksv_key_params {
    ksv_runs R;
    uint32_t n_cols;
    const uint8_t* a[2];              // [n] x 32: the items' scalars of point column 0 / 1
    uint8_t* head[2];                 // [n_keys] x 32
    uint8_t* cell[2];                 // [ksv_cells(n)] x 32
    const uint8_t* key_flags[2];
    const uint32_t* tables[2];
    uint32_t* points;                 // one extended point per block of ksv_key_kernel
};

// the keyed per-item pass
__global__ __launch_bounds__(BLOCK, 2) void ksv_item_kernel(ksv_params B) {
    verdict_item_pass(B, [](const ksv_params& b, uint64_t item, words8* zu) { return ksv_item(b, item, zu); });
}

// the pieces of the runs: per point column, one lane per key (its head) and one per line (its cell)
__global__ __launch_bounds__(BLOCK) void ksv_run_kernel(ksv_key_params S) {
    const uint32_t cells = ksv_cells(S.R.n), units = S.R.n_keys + cells;
    const uint64_t total = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t id = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; id < (uint64_t)S.n_cols * units; id += total) {
        const bool second = id >= units;
        const uint32_t unit = (uint32_t)(second ? id - units : id);
        const uint8_t* a = second ? S.a[1] : S.a[0];
        if (unit < S.R.n_keys) store_words(second ? S.head[1] : S.head[0], unit, ksv_head(S.R, a, unit));
        else store_words(second ? S.cell[1] : S.cell[0], unit - S.R.n_keys, ksv_cell(S.R, a, unit - S.R.n_keys));
    }
}

// S_k * P_k: one lane per (point column, key); the points of a block added by a tree, one point per block
__global__ __launch_bounds__(BLOCK, 2) void ksv_key_kernel(ksv_key_params S) {
    __shared__ uint32_t red[BLOCK * MSM_EXT_WORDS];
    const uint64_t id = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ext_pt acc = ext_identity();
    if (id < (uint64_t)S.n_cols * S.R.n_keys) {
        const bool second = id >= S.R.n_keys;
        key_column C{};
        C.key_flags = const_cast<uint8_t*>(second ? S.key_flags[1] : S.key_flags[0]);
        C.tables = const_cast<uint32_t*>(second ? S.tables[1] : S.tables[0]);
        acc = ksv_key_point(S.R, C, second ? S.head[1] : S.head[0], second ? S.cell[1] : S.cell[0],
                            (uint32_t)(second ? id - S.R.n_keys : id));
    }
    block_sum_ext(red, acc);
    if (threadIdx.x < MSM_EXT_WORDS) S.points[(size_t)blockIdx.x * MSM_EXT_WORDS + threadIdx.x] = red[threadIdx.x];
}

// one block: the per-block sums of z u added, the blocks' key points added, the windows of the R terms combined, the
// fixed-base part, the verdict word
__global__ __launch_bounds__(BLOCK) void ksv_final_kernel(ksv_params B, msm_params M, uint32_t blocks, const uint32_t* points,
                                                          uint32_t point_blocks, uint32_t* verdict) {
    __shared__ uint32_t pts[BLOCK * MSM_EXT_WORDS];
    words8 zu[2];
    verdict_sum_partials(B.partial, blocks, zu);
    ext_pt sum = ext_identity();
    for (uint32_t b = threadIdx.x; b < point_blocks; b += BLOCK) sum = msm_add_ext(sum, msm_load_ext(points + (size_t)b * MSM_EXT_WORDS));
    block_sum_ext(pts, sum);
    if (threadIdx.x == 0) {
        const ext_pt total = msm_add_ext(msm_combine(M.win, M.W, M.c), msm_load_ext(pts));
        *verdict = bv_verdict(B.V, total, zu, *B.fail != 0u) ? 1u : 0u;
    }
}

#if defined(JJS_PROFILING)
// jjs_debug_keyset_sums_dev (include/jjs_gpu_profiling.h): S_k of every (point column, key), 32 bytes each, and, from one
// lane, the sum of the blocks' key points
__global__ __launch_bounds__(BLOCK) void dbg_ksv_sums_kernel(ksv_key_params S, uint32_t point_blocks, uint8_t* sums_out, uint32_t* point_out) {
    const uint64_t id = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (id < (uint64_t)S.n_cols * S.R.n_keys) {
        const bool second = id >= S.R.n_keys;
        store_words(sums_out, id, ksv_key_sum(S.R, second ? S.head[1] : S.head[0], second ? S.cell[1] : S.cell[0],
                                              (uint32_t)(second ? id - S.R.n_keys : id)));
    }
    if (id == 0) {
        ext_pt sum = ext_identity();
        for (uint32_t b = 0; b < point_blocks; ++b) sum = msm_add_ext(sum, msm_load_ext(S.points + (size_t)b * MSM_EXT_WORDS));
        msm_store_ext(point_out, sum);
    }
}
#endif

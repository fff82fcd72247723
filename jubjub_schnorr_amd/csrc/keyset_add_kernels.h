// Part of jjs_gpu.hip (included inside its anonymous namespace, behind every other kernel: the kernels that were there keep
// their places in the code object): the kernels of jjs_keyset_add.  Their bodies are the JJS_HD stage functions of keyset_add.h.
#pragma once
// Adding keys to a live set (keyset_add.h).  The new ids [first, T.n_keys) enter the set's lookup table with their global ids ...
__global__ __launch_bounds__(BLOCK) void keyset_lookup_insert_range_kernel(keyset_lookup T, uint32_t first) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < T.n_keys - first) kl_insert(T, first + t);
}
// ... and the plan of JJS_KEYSET_ADD_UNIQUE, one lane per candidate: probe; claim; mark, with the block's count of first
// occurrences; the scan of the block counts on one block; gather; and, behind the flags of the new range, the answers.
__global__ __launch_bounds__(BLOCK) void keyset_add_probe_kernel(keyset_add_plan P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P.n) ka_probe(P, i);
}
__global__ __launch_bounds__(BLOCK) void keyset_add_claim_kernel(keyset_add_plan P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P.n) ka_claim(P, i);
}
__global__ __launch_bounds__(BLOCK) void keyset_add_mark_kernel(keyset_add_plan P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t f = i < P.n ? ka_mark(P, i) : 0u;
    const int count = __syncthreads_count((int)f);
    if (threadIdx.x == 0) P.sums[blockIdx.x] = (uint32_t)count;
}
__global__ __launch_bounds__(KA_SCAN_LANES) void keyset_add_scan_kernel(uint32_t* sums, uint32_t blocks) {
    __shared__ uint32_t part[KA_SCAN_LANES];
    const uint32_t j = threadIdx.x;
    part[j] = ka_scan_chunk_total(sums, blocks, j);
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (uint32_t k = 0; k < KA_SCAN_LANES; ++k) {       // 256 additions from LDS per lane: nothing beside the chunk passes
        if (k == j) base = total;
        total += part[k];
    }
    ka_scan_chunk_write(sums, blocks, j, base);
    if (j == 0) sums[blocks] = total;
}
__global__ __launch_bounds__(BLOCK) void keyset_add_gather_kernel(keyset_add_plan P) {
    __shared__ uint32_t wave_count[BLOCK / 64];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool f = i < P.n && P.first[i] != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!f) return;
    uint32_t rank = P.sums[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_count[w];
    ka_gather(P, i, rank);
}
__global__ __launch_bounds__(BLOCK) void keyset_add_retract_kernel(uint32_t* slots, uint32_t n_slots, uint32_t n_old) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_slots) ka_retract(slots, i, n_old);
}
// flags0 (flags1): those of the set the candidates were added to, from index 0
__global__ __launch_bounds__(BLOCK) void keyset_add_answer_kernel(keyset_add_plan P, const uint8_t* flags0, const uint8_t* flags1, uint32_t* idx_out,
                                                                  uint8_t* status_out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t idx = ka_index(P, i);
    idx_out[i] = idx;
    status_out[i] = (uint8_t)ka_status(idx, P.C.n_cols, flags0, flags1);
}

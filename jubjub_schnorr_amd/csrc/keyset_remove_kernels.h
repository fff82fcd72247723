// Part of jjs_gpu.hip (included inside its anonymous namespace, behind every other kernel -- keyset_add_kernels.h included: the
// kernels that were there keep their places in the code object): the kernels of jjs_keyset_remove and jjs_keyset_compact.  Their
// bodies are the JJS_HD stage functions of keyset_remove.h.
#pragma once
// Remove, one lane per candidate and launch by launch: the answers; the flag bytes and the counts; the retractions; then one
// lane per id of the set re-enters the higher duplicates of what was retracted.
__global__ __launch_bounds__(BLOCK) void keyset_remove_answer_kernel(keyset_remove_plan P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P.n) kr_answer(P, i);
}
__global__ __launch_bounds__(BLOCK) void keyset_remove_flags_kernel(keyset_remove_plan P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P.n) kr_flags(P, i);
}
__global__ __launch_bounds__(BLOCK) void keyset_remove_retract_kernel(keyset_remove_plan P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P.n) kr_retract(P, i);
}
__global__ __launch_bounds__(BLOCK) void keyset_remove_reenter_kernel(keyset_lookup T) {
    const uint32_t id = blockIdx.x * BLOCK + threadIdx.x;
    if (id < T.n_keys) kr_reenter(T, id);
}
// keyset_miss_kernel for a set that has been removed from: a found index that carries KT_KEY_REMOVED is a miss too.
__global__ __launch_bounds__(BLOCK) void keyset_miss_removed_kernel(const uint32_t* found, uint64_t n, uint8_t* status, unsigned long long* tally,
                                                                    uint32_t n_keys, const uint8_t* flags0) {
    const uint64_t item = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t st = 0;
    const bool miss = item < n && (kl_take_miss(found, item, status, &st) || kr_take_removed(found, item, n_keys, flags0, status, &st));
    if (!tally) return;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const unsigned long long lanes = __ballot(miss && st == k);
        if (lanes && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)lanes) - 1))
            atomicAdd(&tally[k], 0ull - (unsigned long long)__popcll(lanes));
    }
}
// Compact: the survivors of each block of BLOCK ids counted (keyset_add_scan_kernel scans the counts), then gathered by ballot
// rank; an id that is gone learns so in the map.
__global__ __launch_bounds__(BLOCK) void keyset_compact_mark_kernel(keyset_compact_plan P) {
    const uint32_t id = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t f = id < P.n_keys ? kc_survives(P, id) : 0u;
    const int count = __syncthreads_count((int)f);
    if (threadIdx.x == 0) P.sums[blockIdx.x] = (uint32_t)count;
}
__global__ __launch_bounds__(BLOCK) void keyset_compact_gather_kernel(keyset_compact_plan P) {
    __shared__ uint32_t wave_count[BLOCK / 64];
    const uint32_t id = blockIdx.x * BLOCK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool f = id < P.n_keys && kc_survives(P, id) != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!f) {
        if (id < P.n_keys) P.map[id] = KR_GONE;
        return;
    }
    uint32_t rank = P.sums[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_count[w];
    kc_gather(P, id, rank);
}
// The table gather, the one kernel of this family that moves bytes in bulk: 204 KB per key and point column, copied, not computed
// again.  One block per (new id, slice of KR_TABLE_SLICE 16-byte units), so that a set of few keys still spreads over the chip;
// every wave loads and stores 1 KB of adjacent bytes per instruction, four loads in flight per lane.
__global__ __launch_bounds__(BLOCK) void keyset_table_gather_kernel(keyset_table_gather G, uint64_t blocks) {
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) kc_table_piece(G, b, threadIdx.x, BLOCK);
}

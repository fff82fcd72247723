// Part of jjs_gpu.hip (included inside its anonymous namespace, behind every other kernel, so that the kernels that were there keep
// their places in the code object): the kernels of jjs_digest* (digest.h, digest_calls.h).
// The pass in front of a call with an item beyond the tag table: one lane per item (a uniform call: one lane) computes its SAFE tag.
__global__ __launch_bounds__(BLOCK) void digest_tags_kernel(digest_params D) {
    const uint64_t total = (uint64_t)gridDim.x * BLOCK, count = D.offsets ? D.n : 1;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < count; i += total) dg_tag_item(D, i);
}
// One lane per item, the throughput route: lane j of the grid takes item order[j] (item j of a uniform call) and strides over
// the grid; the trip's first lane is wave-uniform, so the loop costs the hash no vector register.  A kernel per format: each keeps
// the registers of its own ingest.  (Held to four waves per SIMD with amdgpu_waves_per_eu the kernels spill 2-4 vector registers,
// whichever of the item's index, the range flag and the element count is folded away: they run at three.)
template <uint32_t FMT>
__global__ __launch_bounds__(BLOCK) void digest_kernel(digest_params D) {
    const uint32_t gtid = blockIdx.x * BLOCK + threadIdx.x, total = gridDim.x * BLOCK;
    for (uint64_t base = 0; base < D.n; base += total)
        if (base + gtid < D.n) dg_lane<FMT>(D, base + gtid, -1, true);
}
// Eight adjacent lanes per item, the latency route (hades_permute, coop).  Whole groups of eight take an item or none, and the
// sponge's loop of a group runs as long as that group's item: the exchanges of a group stay inside it.
template <uint32_t FMT>
__global__ __launch_bounds__(BLOCK) void digest_coop_kernel(digest_params D) {
    const uint32_t gtid = blockIdx.x * BLOCK + threadIdx.x, total = gridDim.x * BLOCK;
    const int coop = (int)(gtid % DG_COOP_LANES);
    for (uint64_t base = 0; base < D.n; base += total / DG_COOP_LANES)
        if (base + gtid / DG_COOP_LANES < D.n) dg_lane<FMT>(D, base + gtid / DG_COOP_LANES, coop, coop == 0);
}

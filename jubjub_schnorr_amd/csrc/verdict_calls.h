// Part of jjs_gpu.hip (included among the extern "C" entry points): the batch verdict (batch_verdict.h, msm.h;
// include/jjs_gpu.h jjs_verify_all_*) -- the routing between the verdict algorithm and the per-item path, the launches
// of the verdict algorithm (its kernels: verdict_kernels.h), and the entry points.

// ---- routing --------------------------------------------------------------------------------------------------------------
// The verdict algorithm runs where it was measured faster than the per-item path and a tally check (DESIGN.md 5f,
// profiles/r06_verify_all.jsonl): from VERDICT_MIN_ITEMS[scheme] items on.  SIZE_MAX: nowhere.  It wins only on batches
// whose keys do not repeat (1.22x single, 1.31x double, 1.43x var-gen at 2^20) and loses 1.7-2.1x at SURVEY 8(d)'s 4 096
// keys; the key class of a batch is found on the device, after the call is queued, so no size alone is safe.
constexpr size_t VERDICT_MIN_ITEMS[3] = {SIZE_MAX, SIZE_MAX, SIZE_MAX};
#if defined(JJS_PROFILING)
static int g_force_verdict = 0;          // jjs_debug_force_path 0x2000: the verdict algorithm at any size; 0x4000: never
static int g_force_msm_window = 0;       // ... bits 16-20: the MSM's window width (0: by size)
static bool g_pin_batch_seed = false;    // jjs_debug_pin_hash_seed(on) with on & 2: the key 00 01 .. 1f
#endif
static bool verdict_route(int scheme, size_t n) {
    const size_t kinds = scheme == JJS_SCHEME_DOUBLE ? 4 : (scheme == JJS_SCHEME_SINGLE ? 2 : 3);
    if (kinds * n >= 0x80000000ull) return false;        // term indices carry a sign bit
#if defined(JJS_PROFILING)
    if (g_force_verdict) return g_force_verdict == 1;
#endif
    return n >= VERDICT_MIN_ITEMS[scheme];
}
static int batch_seed(uint32_t seed[8]) {
#if defined(JJS_PROFILING)
    if (g_pin_batch_seed) {
        for (int i = 0; i < 8; ++i) seed[i] = 0x03020100u + 0x04040404u * (uint32_t)i;
        return JJS_OK;
    }
#endif
    uint8_t* p = reinterpret_cast<uint8_t*>(seed);
    size_t got = 0;
    while (got < 32) {
        const ssize_t r = getrandom(p + got, 32 - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return fail(JJS_ERR_HIP, "getrandom failed: errno %d", errno);
        }
        got += (size_t)r;
    }
    return JJS_OK;
}

static verify_params verdict_params(int scheme, const void* const* d, size_t n) {
    const uint8_t* const* p = reinterpret_cast<const uint8_t* const*>(d);
    const out_ptrs o{nullptr, nullptr, nullptr, nullptr};
    if (scheme == JJS_SCHEME_SINGLE) return scheme_params(scheme, p[0], p[1], nullptr, p[2], nullptr, p[3], n, o);
    if (scheme == JJS_SCHEME_DOUBLE) return scheme_params(scheme, p[0], p[1], p[2], p[3], p[4], p[5], n, o);
    return scheme_params(scheme, p[0], p[1], nullptr, p[2], p[3], p[4], n, o);
}

// ---- the MSM of a verdict call (msm.h; its kernels: verdict_kernels.h) --------------------------------------------------------
// the window width: by size, or jjs_debug_force_path's
static int msm_window(int by_size) {
#if defined(JJS_PROFILING)
    if (g_force_msm_window >= 8 && g_force_msm_window <= MSM_MAX_WINDOW) return g_force_msm_window;
#endif
    return by_size;
}
extern "C++" {
// The slot's verdict scratch of a call whose item pass runs `blocks` blocks (B: bv_params or ksv_params; M: its n, N and
// shape set), sized and carved: the fail word with the scan's span sums behind it (<= 4096 + 1 words), the item pass's
// partial sums, the terms, the scalars, M.off .. M.win, then the caller's n_extra parts of extra[i] bytes (-> q_extra[i]),
// each part padded to 256 bytes.
constexpr int MSM_PARTS = 10;
template <class P>
static int verdict_scratch(P& B, msm_params& M, uint32_t blocks, const size_t* extra, int n_extra, uint8_t** q_extra, uint32_t*& span_sum) {
    const size_t nb = (size_t)M.W * M.B;
    const size_t sz[MSM_PARTS] = {64 + 4 * ((nb + MSM_SCAN_SPAN - 1) / MSM_SCAN_SPAN + 1), (size_t)blocks * 64, M.N * MSM_TERM_WORDS * 4, M.N * 32,
                                  (nb + 1) * 4, nb * 4, M.N * M.W * 4, nb * MSM_EXT_WORDS * 4, (size_t)M.W * M.K * MSM_EXT_WORDS * 4,
                                  (size_t)M.W * MSM_EXT_WORDS * 4};
    size_t total = 0;
    for (size_t x : sz) total += pad256(x);
    for (int i = 0; i < n_extra; ++i) total += pad256(extra[i]);
    if (int rc = sl->verdict.ensure(total)) return rc;
    uint8_t* p = sl->verdict;
    uint8_t* q[MSM_PARTS];
    for (int i = 0; i < MSM_PARTS; ++i) { q[i] = p; p += pad256(sz[i]); }
    for (int i = 0; i < n_extra; ++i) { q_extra[i] = p; p += pad256(extra[i]); }
    B.fail = reinterpret_cast<uint32_t*>(q[0]);
    span_sum = B.fail + 16;
    B.partial = q[1];
    B.terms = reinterpret_cast<uint32_t*>(q[2]);
    B.scalars = q[3];
    M.terms = B.terms; M.scalars = B.scalars;
    M.off = reinterpret_cast<uint32_t*>(q[4]); M.cursor = reinterpret_cast<uint32_t*>(q[5]); M.order = reinterpret_cast<uint32_t*>(q[6]);
    M.buckets = reinterpret_cast<uint32_t*>(q[7]); M.segs = reinterpret_cast<uint32_t*>(q[8]); M.win = reinterpret_cast<uint32_t*>(q[9]);
    return JJS_OK;
}
}  // extern "C++"
// the MSM's launches on stream s, after the item pass has written the terms and scalars and M.off is clear
static void msm_launch(const msm_params& M, uint32_t* span_sum, hipStream_t s) {
    const size_t nb = (size_t)M.W * M.B;
    const unsigned term_blocks = (unsigned)grid_for(8192, M.N);
    hipLaunchKernelGGL(msm_sort_kernel<false>, dim3(term_blocks), dim3(BLOCK), 0, s, M);
    const unsigned spans = (unsigned)((nb + MSM_SCAN_SPAN - 1) / MSM_SCAN_SPAN);
    hipLaunchKernelGGL(msm_scan_kernel<0>, dim3(spans), dim3(1024), 0, s, M, span_sum);
    hipLaunchKernelGGL(msm_scan_kernel<1>, dim3(1), dim3(1024), 0, s, M, span_sum);
    hipLaunchKernelGGL(msm_scan_kernel<2>, dim3(spans), dim3(1024), 0, s, M, span_sum);
    hipLaunchKernelGGL(msm_sort_kernel<true>, dim3(term_blocks), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(msm_bucket_kernel, dim3((unsigned)((nb + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(msm_segment_kernel, dim3((unsigned)(((size_t)M.W * M.K + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(msm_window_kernel, dim3((unsigned)M.W), dim3(BLOCK), 0, s, M);
}

// The front of the verdict algorithm on stream s (under L.mu; g is the device), up to and including the item pass: the
// descriptor over d = the affine columns in the entry point's order, the seed, the MSM's shape (window: its width, 0 = by
// size), the slot and its scratch, the clear, bv_item_kernel over `blocks` blocks (0: the call's own grid).  It returns with the
// slot shared (begin_shared): the caller queues what reads the scratch and ends with end_shared.
struct verdict_front {
    bv_params B;
    msm_params M;
    uint32_t blocks;
    uint32_t* span_sum;
};
static int verdict_front_launch(int scheme, const void* const* d, size_t n, int window, uint32_t blocks, hipStream_t s, verdict_front& F) {
    bv_params& B = F.B;
    msm_params& M = F.M;
    B = bv_params{};
    B.V = verdict_params(scheme, d, n);
    if (int rc = batch_seed(B.seed)) return rc;
    B.n_kinds = bv_kinds(B.V);
    M = msm_params{};
    M.n = n; M.N = (uint64_t)B.n_kinds * n;
    for (uint32_t k = 0; k < B.n_kinds; ++k) M.neg_kinds |= bv_kind_negated(B.V, k) ? 1u << k : 0u;
    static_cast<msm_shape&>(M) = msm_shape_full(window ? window : msm_window(msm_pick_window(M.N)));
    B.z_bits = msm_weight_bits(M.c);
    F.blocks = blocks ? blocks : (uint32_t)grid_for(g->grid_prepare, n);
    pick_slot(n, s);
    F.span_sum = nullptr;
    if (int rc = verdict_scratch(B, M, F.blocks, nullptr, 0, nullptr, F.span_sum)) return rc;
    if (int rc = begin_shared(s)) return rc;
    const size_t nb = (size_t)M.W * M.B;
    clear_params Z{};
    Z.p[0] = B.fail; Z.bytes[0] = 4;
    Z.p[1] = M.off; Z.bytes[1] = (nb + 1) * 4;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)grid_for(256, nb / 16 + 1)), dim3(BLOCK), 0, s, Z);
    hipLaunchKernelGGL(bv_item_kernel, dim3(F.blocks), dim3(BLOCK), 0, s, B);
    return JJS_OK;
}
// The verdict algorithm on stream s (under L.mu; g is the device): d = the affine columns in the entry point's order.
static int verdict_launch_msm(int scheme, const void* const* d, size_t n, uint32_t* verdict, hipStream_t s) {
    verdict_front F;
    if (int rc = verdict_front_launch(scheme, d, n, 0, 0, s, F)) return rc;
    msm_launch(F.M, F.span_sum, s);
    hipLaunchKernelGGL(bv_final_kernel, dim3(1), dim3(BLOCK), 0, s, F.B, F.M, F.blocks, verdict);
    HIP_TRY(hipGetLastError());
    return end_shared(s);
}
// The per-item route on stream s (under L.mu): the resident call with its tally in the slot, then the verdict from the tally.
static int verdict_launch_items(int scheme, const void* const* d, size_t n, uint32_t* verdict, hipStream_t s) {
    staged_call C;
    if (int rc = build_call(SHAPES[scheme][JJS_FORMAT_AFFINE], d, n, nullptr, nullptr, s, C)) return rc;
    if (int rc = sl->verdict.ensure(256)) return rc;
    unsigned long long* tally = reinterpret_cast<unsigned long long*>(sl->verdict.get());
    C.P.tally = tally;
    if (int rc = launch_staged(C, s)) return rc;
    hipLaunchKernelGGL(tally_verdict_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)tally, (uint64_t)n, verdict);
    HIP_TRY(hipGetLastError());
    return end_shared(s);                       // the slot's tally is read until here
}
static size_t verdict_cols(int scheme) { return scheme == JJS_SCHEME_DOUBLE ? 6 : (scheme == JJS_SCHEME_SINGLE ? 4 : 5); }

// the verdict word of a resident call, checked; an empty batch is answered here (1)
static int verdict_word_dev(void* verdict, size_t n, hipStream_t s) {
    if (!verdict || (reinterpret_cast<uintptr_t>(verdict) & 3u)) return fail(JJS_ERR_ARG, "null or misaligned verdict word");
    if (n == 0) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)verdict, 1, 1, s));
    return JJS_OK;
}
// a resident verdict call: device columns d[], the verdict word on the device, asynchronous on `stream`
static int verdict_dev(int scheme, const void* const* d, size_t n, void* verdict, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = verdict_word_dev(verdict, n, s)) return rc;
    if (n == 0) return JJS_OK;
    for (size_t k = 0; k < verdict_cols(scheme); ++k)
        if (!d[k] || !aligned16(d[k])) return fail(JJS_ERR_ARG, "null or misaligned input pointer");
    return no_throw([&] {
        return verdict_route(scheme, n) ? verdict_launch_msm(scheme, d, n, (uint32_t*)verdict, s)
                                        : verdict_launch_items(scheme, d, n, (uint32_t*)verdict, s);
    });
}

// The verdict algorithm's route of a blocking host call that has counted itself among g_blocking_calls: the columns go
// whole to dev's key-set staging area (one such call at a time per device, host_mu), launch(k, c, d, verdict word, stream)
// runs under L.mu, the verdict comes back.  Verdict 1: every status is 0; verdict 0: the statuses come from per_item().
extern "C++" {
template <class Launch, class PerItem>
static int verdict_host_msm(device_state* dev, const jjs_keyset* ks, const size_t* widths, const void* const* src, size_t cols, size_t n,
                            Launch launch, PerItem per_item, uint8_t* status, int* verdict) {
    int v = 0;
    {
        blocking_call_leave leave_on_every_way_out;
        std::lock_guard<std::mutex> big(dev->host_mu);
        g = dev;
        int rc = no_throw([&]() -> int {
            const size_t out_bytes[1] = {256};                        // the verdict word
            keyset_stage S{};
            if (int r = keyset_stage_in(dev, widths, src, cols, n, out_bytes, 1, S)) return r;
            uint32_t* vw = reinterpret_cast<uint32_t*>(S.out[0]);
            if (int r = keyset_launch_locked(dev, ks, [&](keyset_entry* k, const keyset_copy* c) { return launch(k, c, S.d, vw, S.s); })) return r;
            uint32_t hv = 0;
            HIP_TRY(hipMemcpyAsync(&hv, vw, 4, hipMemcpyDeviceToHost, S.s));
            HIP_TRY(hipStreamSynchronize(S.s));
            v = hv ? 1 : 0;
            return JJS_OK;
        });
        if (rc) return rc;
    }
    *verdict = v;
    if (status) {
        if (v) memset(status, 0, n);
        else return per_item();
    }
    return JJS_OK;
}
}  // extern "C++"

// a host-buffer verdict call: blocking.  The per-item route is the existing host call (its statuses are the caller's).
static int verdict_host(int scheme, const uint8_t* const* ptrs, size_t n, uint8_t* status, int* verdict) {
    if (!verdict) return fail(JJS_ERR_ARG, "null verdict");
    const size_t ncol = verdict_cols(scheme);
    for (size_t k = 0; k < ncol; ++k)
        if (n && !ptrs[k]) return fail(JJS_ERR_ARG, "null input pointer");
    device_state* dev = nullptr;
    bool msm = false;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        if (n == 0) { *verdict = 1; return JJS_OK; }
        msm = L.devs.size() == 1 && verdict_route(scheme, n);
        dev = g;
        if (msm) ++g_blocking_calls;       // jjs_shutdown does not free `dev` before this call has left
    }
    uint64_t tally[4] = {};
    auto per_item = [&] { return host_call(scheme, JJS_FORMAT_AFFINE, ptrs, n, status, tally); };
    if (!msm) {
        if (int rc = per_item()) return rc;
        *verdict = tally[0] == n ? 1 : 0;
        return JJS_OK;
    }
    size_t widths[6];
    for (size_t i = 0; i < ncol; ++i) widths[i] = SHAPES[scheme][JJS_FORMAT_AFFINE].col[i].width;
    return verdict_host_msm(dev, nullptr, widths, reinterpret_cast<const void* const*>(ptrs), ncol, n,
                            [&](keyset_entry*, const keyset_copy*, const void* const* d, uint32_t* vw, hipStream_t s) {
                                return verdict_launch_msm(scheme, d, n, vw, s);
                            },
                            per_item, status, verdict);
}

extern "C" {

int jjs_verify_all_single(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* m, size_t n, uint8_t* status,
                          int* verdict) {
    const uint8_t* p[] = {u, R, PK, m};
    return verdict_host(JJS_SCHEME_SINGLE, p, n, status, verdict);
}
int jjs_verify_all_double(const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PKp,
                          const uint8_t* m, size_t n, uint8_t* status, int* verdict) {
    const uint8_t* p[] = {u, R, Rp, PK, PKp, m};
    return verdict_host(JJS_SCHEME_DOUBLE, p, n, status, verdict);
}
int jjs_verify_all_vargen(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* Gen, const uint8_t* m, size_t n,
                          uint8_t* status, int* verdict) {
    const uint8_t* p[] = {u, R, PK, Gen, m};
    return verdict_host(JJS_SCHEME_VARGEN, p, n, status, verdict);
}
int jjs_verify_all_single_dev(const void* u, const void* R, const void* PK, const void* m, size_t n, void* verdict, void* stream) {
    const void* d[] = {u, R, PK, m};
    return verdict_dev(JJS_SCHEME_SINGLE, d, n, verdict, stream);
}
int jjs_verify_all_double_dev(const void* u, const void* R, const void* Rp, const void* PK, const void* PKp, const void* m, size_t n,
                              void* verdict, void* stream) {
    const void* d[] = {u, R, Rp, PK, PKp, m};
    return verdict_dev(JJS_SCHEME_DOUBLE, d, n, verdict, stream);
}
int jjs_verify_all_vargen_dev(const void* u, const void* R, const void* PK, const void* Gen, const void* m, size_t n, void* verdict,
                              void* stream) {
    const void* d[] = {u, R, PK, Gen, m};
    return verdict_dev(JJS_SCHEME_VARGEN, d, n, verdict, stream);
}

#if defined(JJS_PROFILING)
// what the item-pass debug entries check: the forced window width and block count, the output pointers
static int debug_items_args(size_t n, uint64_t terms, int c, unsigned blocks, const void* scalars_out, const void* partial_out, const void* fail_out,
                            const void* zu_out, const unsigned* blocks_out) {
    if (n == 0 || terms >= 0x80000000ull) return fail(JJS_ERR_ARG, "the item count is out of range");
    if (c < 8 || c > MSM_MAX_WINDOW) return fail(JJS_ERR_ARG, "the window width is out of range");
    if (blocks > 65536u) return fail(JJS_ERR_ARG, "the block count is out of range");
    if (!all_ok(scalars_out, partial_out, fail_out, zu_out) || !blocks_out) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    return JJS_OK;
}
// ... and what they copy out behind the item pass: the scalars, the blocks' partial sums, the fail word, then the final
// kernels' sum of the partial sums from one block
static int debug_items_out(const uint8_t* scalars, size_t scalar_bytes, const uint8_t* partial, uint32_t blocks, const uint32_t* fail_word,
                           void* scalars_out, void* partial_out, void* fail_out, void* zu_out, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(scalars_out, scalars, scalar_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(partial_out, partial, (size_t)blocks * 64, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(fail_out, fail_word, 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(dbg_verdict_totals_kernel, dim3(1), dim3(BLOCK), 0, s, partial, blocks, (uint8_t*)zu_out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
// include/jjs_gpu_profiling.h: the item pass of a verdict call -- verdict_front_launch, as verdict_launch_msm runs it -- with
// what it wrote copied out
int jjs_debug_verdict_items_dev(int scheme, const void* d0, const void* d1, const void* d2, const void* d3, const void* d4, const void* d5,
                                size_t n, int c, unsigned blocks, void* scalars_out, void* partial_out, void* fail_out, void* zu_out,
                                unsigned* blocks_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (scheme < 0 || scheme > 2) return fail(JJS_ERR_ARG, "scheme out of range");
    if (int rc = debug_items_args(n, 4ull * n, c, blocks, scalars_out, partial_out, fail_out, zu_out, blocks_out)) return rc;
    const void* d[] = {d0, d1, d2, d3, d4, d5};
    for (size_t k = 0; k < verdict_cols(scheme); ++k)
        if (!all_ok(d[k])) return fail(JJS_ERR_ARG, "null or misaligned input pointer");
    hipStream_t s = (hipStream_t)stream;
    return no_throw([&]() -> int {
        verdict_front F;
        if (int rc = verdict_front_launch(scheme, d, n, c, blocks, s, F)) return rc;
        *blocks_out = F.blocks;
        const int rc = debug_items_out(F.B.scalars, (size_t)F.M.N * 32, F.B.partial, F.blocks, F.B.fail, scalars_out, partial_out, fail_out, zu_out, s);
        const int rc2 = end_shared(s);
        return rc ? rc : rc2;
    });
}
// include/jjs_gpu_profiling.h: the MSM of a verdict call over the caller's own terms -- verdict_scratch, the calls' clear,
// msm_launch -- with every stage's output copied out
int jjs_debug_msm_dev(const void* points, const void* scalars, size_t n, unsigned n_kinds, unsigned neg_kinds, int c, int short_shape,
                      void* off_out, void* order_out, void* win_out, void* total_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0 || n_kinds < 1 || n_kinds > 4 || (uint64_t)n_kinds * n >= 0x80000000ull) return fail(JJS_ERR_ARG, "the term count is out of range");
    if (c < 8 || c > MSM_MAX_WINDOW) return fail(JJS_ERR_ARG, "the window width is out of range");
    if (!all_ok(points, scalars, off_out, order_out, win_out, total_out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    return no_throw([&]() -> int {
        bv_params B{};
        msm_params M{};
        M.n = n; M.N = (uint64_t)n_kinds * n;
        M.neg_kinds = neg_kinds & ((1u << n_kinds) - 1u);
        static_cast<msm_shape&>(M) = short_shape ? msm_shape_short(c) : msm_shape_full(c);
        pick_slot(n, s);
        uint32_t* span_sum = nullptr;
        if (int rc = verdict_scratch(B, M, 1, nullptr, 0, nullptr, span_sum)) return rc;
        if (int rc = begin_shared(s)) return rc;
        const size_t nb = (size_t)M.W * M.B;
        clear_params Z{};
        Z.p[0] = B.fail; Z.bytes[0] = 4;
        Z.p[1] = M.off; Z.bytes[1] = (nb + 1) * 4;
        hipLaunchKernelGGL(clear_kernel, dim3((unsigned)grid_for(256, nb / 16 + 1)), dim3(BLOCK), 0, s, Z);
        hipLaunchKernelGGL(dbg_msm_terms_kernel, dim3((unsigned)((M.N + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, (const uint8_t*)points,
                           (const uint8_t*)scalars, M.N, B.terms, B.scalars);
        msm_launch(M, span_sum, s);
        hipLaunchKernelGGL(dbg_msm_out_kernel, dim3((unsigned)grid_for(256, nb + 1)), dim3(BLOCK), 0, s, M, (uint32_t*)off_out, (uint32_t*)order_out,
                           (uint32_t*)win_out, (uint32_t*)total_out);
        HIP_TRY(hipGetLastError());
        return end_shared(s);
    });
}
#endif

}  // extern "C"

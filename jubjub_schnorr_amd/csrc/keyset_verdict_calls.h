// Part of jjs_gpu.hip (included among the extern "C" entry points, after keyset_calls.h and verdict_calls.h): the batch
// verdict against a registered key set (keyset_verdict.h; include/jjs_gpu.h jjs_keyset_verify_all*) -- the routing between
// the verdict algorithm and the per-item key-set call, the launches of the verdict algorithm (its kernels:
// keyset_verdict_kernels.h and the MSM's in verdict_kernels.h), and the entry points.

// ---- routing --------------------------------------------------------------------------------------------------------------
// The verdict algorithm runs where profiles/r07_keyset_verify_all.jsonl has it faster than the per-item call with a tally
// check, by more than either side's spread, at every key count measured and on the one-key batch: from
// KEYSET_VERDICT_MIN_ITEMS[scheme] items on.  SIZE_MAX: nowhere.  Signatures in the ext and wire formats always take the
// per-item route (their decode / normalise stage writes into the per-item call's own descriptor).
constexpr size_t KEYSET_VERDICT_MIN_ITEMS[3] = {SIZE_MAX, SIZE_MAX, SIZE_MAX};
static bool keyset_verdict_route(int scheme, int format, size_t n) {
    if (format != JJS_FORMAT_AFFINE) return false;
    if ((scheme == JJS_SCHEME_DOUBLE ? 2 : 1) * n >= 0x80000000ull) return false;        // term indices carry a sign bit
#if defined(JJS_PROFILING)
    if (g_force_verdict) return g_force_verdict == 1;
#endif
    return n >= KEYSET_VERDICT_MIN_ITEMS[scheme];
}

// The verdict algorithm on stream s (under L.mu; g is c's device): d = key_idx, u, R, R', m (device, affine signatures).
static int keyset_verdict_launch_msm(keyset_entry& k, const keyset_copy& c, const void* const* d, size_t n, uint32_t* verdict, hipStream_t s) {
    const int scheme = k.scheme;
    ksv_params B{};
    if (int rc = batch_seed(B.seed)) return rc;
    pick_slot(n, s);
    if (int rc = ensure_wire(n)) return rc;
    const uint32_t stride = k.n_keys < CURSOR_DENSE_FROM ? CURSOR_STRIDE : 1u;
    const size_t cursor_words = (size_t)k.n_keys + 1 > (size_t)CURSOR_DENSE_FROM * CURSOR_STRIDE ? (size_t)k.n_keys + 1
                                                                                                  : (size_t)CURSOR_DENSE_FROM * CURSOR_STRIDE;
    if (int rc = ensure_key_index(2 * pad256(n * 4) + pad256(cursor_words * 4))) return rc;
    const out_ptrs o{nullptr, nullptr, nullptr, nullptr};
    const uint8_t *u = (const uint8_t*)d[1], *R = (const uint8_t*)d[2], *Rp = (const uint8_t*)d[3], *m = (const uint8_t*)d[4];
    if (scheme == JJS_SCHEME_SINGLE) B.V = params_single(u, R, wire_pts(2), m, n, g->comb_g, o);
    else if (scheme == JJS_SCHEME_DOUBLE) B.V = params_double(u, R, Rp, wire_pts(2), wire_pts(3), m, n, g->tag, g->comb_g, g->comb_gn, o);
    else B.V = params_vargen(u, R, wire_pts(2), wire_pts(3), m, n, o);
    B.V.pre_malformed = wire_bad();
    B.V.key_flag = c.words + 2;
    B.n_cols = k.n_cols;
    key_params K{};
    K.n_cols = k.n_cols; K.max_keys = k.n_keys; K.max_keys_wide = k.n_keys; K.n = n; K.counters = c.words;
    uint8_t* kq = sl->keys;
    uint32_t* keyid = reinterpret_cast<uint32_t*>(kq); kq += pad256(n * 4);
    K.order = reinterpret_cast<uint32_t*>(kq); kq += pad256(n * 4);
    K.key_cursor = reinterpret_cast<uint32_t*>(kq);
    K.col[0].keyid = keyid;
    B.keyid = keyid;
    for (uint32_t i = 0; i < k.n_cols; ++i) B.key_flags[i] = c.flags[i];

    msm_params M{};
    M.n = n; M.N = (uint64_t)B.V.n_eq * n;
    M.neg_kinds = (1u << B.V.n_eq) - 1u;                 // every term is a -R
    M.c = msm_pick_short_window(M.N);
#if defined(JJS_PROFILING)
    if (g_force_msm_window >= 8 && g_force_msm_window <= MSM_MAX_WINDOW) M.c = g_force_msm_window;
#endif
    B.z_bits = msm_weight_bits(M.c);
    M.W = msm_short_windows(M.c); M.top_split = 0; M.B = msm_buckets(M.c); M.K = msm_short_segments(M.c); M.L = M.B / M.K;
    const uint32_t blocks = (uint32_t)grid_for(g->grid_prepare, n);
    const uint32_t cells = ksv_cells(n), point_blocks = (uint32_t)(((uint64_t)k.n_cols * k.n_keys + BLOCK - 1) / BLOCK);
    const size_t nb = (size_t)M.W * M.B, second = k.n_cols > 1 ? 1 : 0;       // (no second point column: no second scalar column)
    const size_t sz[] = {pad256(64 + 4 * ((nb + MSM_SCAN_SPAN - 1) / MSM_SCAN_SPAN + 1)), pad256((size_t)blocks * 64), pad256(M.N * MSM_TERM_WORDS * 4),
                         pad256(M.N * 32), pad256((nb + 1) * 4), pad256(nb * 4), pad256(M.N * M.W * 4), pad256(nb * MSM_EXT_WORDS * 4),
                         pad256((size_t)M.W * M.K * MSM_EXT_WORDS * 4), pad256((size_t)M.W * MSM_EXT_WORDS * 4),
                         pad256(n * 32), pad256(second * n * 32), pad256((size_t)k.n_keys * 32), pad256(second * k.n_keys * 32),
                         pad256((size_t)cells * 32), pad256(second * cells * 32), pad256((size_t)point_blocks * MSM_EXT_WORDS * 4)};
    constexpr int parts = sizeof(sz) / sizeof(sz[0]);
    size_t total = 0;
    for (size_t x : sz) total += x;
    if (int rc = ensure_verdict(total)) return rc;
    uint8_t* p = sl->verdict;
    uint8_t* q[parts];
    for (int i = 0; i < parts; ++i) { q[i] = p; p += sz[i]; }
    B.fail = reinterpret_cast<uint32_t*>(q[0]);
    B.partial = q[1];
    B.terms = reinterpret_cast<uint32_t*>(q[2]);
    B.scalars = q[3];
    M.terms = B.terms; M.scalars = B.scalars;
    M.off = reinterpret_cast<uint32_t*>(q[4]); M.cursor = reinterpret_cast<uint32_t*>(q[5]); M.order = reinterpret_cast<uint32_t*>(q[6]);
    M.buckets = reinterpret_cast<uint32_t*>(q[7]); M.segs = reinterpret_cast<uint32_t*>(q[8]); M.win = reinterpret_cast<uint32_t*>(q[9]);
    B.a[0] = q[10]; B.a[1] = q[11];
    ksv_key_params S{};
    S.R = ksv_runs{K.key_cursor, stride, K.order, keyid, k.n_keys, n};
    S.n_cols = k.n_cols;
    for (int i = 0; i < 2; ++i) {
        S.a[i] = B.a[i]; S.head[i] = q[12 + i]; S.cell[i] = q[14 + i];
        S.key_flags[i] = c.flags[i]; S.tables[i] = c.tables[i];
    }
    S.points = reinterpret_cast<uint32_t*>(q[16]);

    if (int rc = begin_shared(s)) return rc;
    clear_params Z{};
    Z.p[0] = B.fail; Z.bytes[0] = 4;
    Z.p[1] = M.off; Z.bytes[1] = (nb + 1) * 4;
    Z.p[2] = wire_bad(); Z.bytes[2] = n;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)grid_for(256, (nb > n ? nb : n) / 16 + 1)), dim3(BLOCK), 0, s, Z);
    keyset_index_params X{};
    X.key_idx = (const uint32_t*)d[0]; X.n_keys = k.n_keys; X.n_cols = k.n_cols;
    X.keys[0] = c.keys[0]; X.keys[1] = c.keys[1]; X.out[0] = wire_pts(2); X.out[1] = wire_pts(3);
    X.keyid = keyid; X.bad = wire_bad(); X.n = n;
    X.cursor = K.key_cursor; X.cursor_words = cursor_words;
    hipLaunchKernelGGL(keyset_index_kernel, dim3((unsigned)grid_for(8192, n > cursor_words ? n : cursor_words)), dim3(BLOCK), 0, s, X);
    const unsigned item_blocks = (unsigned)grid_for(8192, n);
    hipLaunchKernelGGL(key_count_kernel, dim3(item_blocks), dim3(BLOCK), 0, s, K);
    hipLaunchKernelGGL(key_scan_kernel, dim3(1), dim3(1024), 0, s, K);
    hipLaunchKernelGGL(key_scatter_kernel, dim3(item_blocks), dim3(BLOCK), 0, s, K);
    hipLaunchKernelGGL(ksv_item_kernel, dim3(blocks), dim3(BLOCK), 0, s, B);
    // the key points: the runs' pieces, then S_k * PK_k over the set's tables
    hipLaunchKernelGGL(ksv_run_kernel, dim3((unsigned)grid_for(8192, (size_t)k.n_cols * (k.n_keys + cells))), dim3(BLOCK), 0, s, S);
    hipLaunchKernelGGL(ksv_key_kernel, dim3(point_blocks), dim3(BLOCK), 0, s, S);
    // the MSM over the R terms
    const unsigned term_blocks = (unsigned)grid_for(8192, M.N);
    hipLaunchKernelGGL(msm_sort_kernel<false>, dim3(term_blocks), dim3(BLOCK), 0, s, M);
    const unsigned spans = (unsigned)((nb + MSM_SCAN_SPAN - 1) / MSM_SCAN_SPAN);
    uint32_t* span_sum = reinterpret_cast<uint32_t*>(q[0]) + 16;        // <= 4096 + 1 words behind the fail word
    hipLaunchKernelGGL(msm_scan_kernel<0>, dim3(spans), dim3(1024), 0, s, M, span_sum);
    hipLaunchKernelGGL(msm_scan_kernel<1>, dim3(1), dim3(1024), 0, s, M, span_sum);
    hipLaunchKernelGGL(msm_scan_kernel<2>, dim3(spans), dim3(1024), 0, s, M, span_sum);
    hipLaunchKernelGGL(msm_sort_kernel<true>, dim3(term_blocks), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(msm_bucket_kernel, dim3((unsigned)((nb + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(msm_segment_kernel, dim3((unsigned)(((size_t)M.W * M.K + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(msm_window_kernel, dim3((unsigned)M.W), dim3(BLOCK), 0, s, M);
    hipLaunchKernelGGL(ksv_final_kernel, dim3(1), dim3(BLOCK), 0, s, B, M, blocks, (const uint32_t*)S.points, point_blocks, verdict);
    HIP_TRY(hipGetLastError());
    return end_shared(s);
}
// The per-item route on stream s (under L.mu): the key-set call with its tally in the slot, then the verdict from the tally.
static int keyset_verdict_launch_items(keyset_entry& k, const keyset_copy& c, int format, const void* const* d, size_t n, uint32_t* verdict,
                                       hipStream_t s) {
    pick_slot(n, s);
    if (int rc = ensure_verdict(256)) return rc;
    unsigned long long* tally = reinterpret_cast<unsigned long long*>(sl->verdict);
    {
        struct keep_slot {                      // keyset_launch picks its slot itself: the one that holds the tally
            call_slot* before = forced_slot;
            keep_slot() { forced_slot = sl; }
            ~keep_slot() { forced_slot = before; }
        } keep;
        if (int rc = keyset_launch(k, c, format, d, n, nullptr, tally, s)) return rc;
    }
    if (int rc = begin_shared(s)) return rc;
    hipLaunchKernelGGL(tally_verdict_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)tally, (uint64_t)n, verdict);
    HIP_TRY(hipGetLastError());
    return end_shared(s);                       // the slot's tally is read until here
}

extern "C" {

int jjs_keyset_verify_all_dev(jjs_keyset ks, int format, const void* key_idx, const void* s0, const void* s1, const void* s2, const void* m,
                              size_t n, void* verdict, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = find_keyset(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    hipStream_t s = (hipStream_t)stream;
    if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
    if (!verdict || (reinterpret_cast<uintptr_t>(verdict) & 3u)) return fail(JJS_ERR_ARG, "null or misaligned verdict word");
    if (n == 0) {
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)verdict, 1, 1, s));
        return JJS_OK;
    }
    if (int rc = keyset_check_cols(k->scheme, format, key_idx, s0, s1, s2, m, true)) return rc;
    const keyset_copy* c = keyset_copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    const void* d[] = {key_idx, s0, s1, s2, m};
    return no_throw([&] {
        return keyset_verdict_route(k->scheme, format, n) ? keyset_verdict_launch_msm(*k, *c, d, n, (uint32_t*)verdict, s)
                                                          : keyset_verdict_launch_items(*k, *c, format, d, n, (uint32_t*)verdict, s);
    });
}

// A host-buffer verdict call: blocking.  The per-item route is jjs_keyset_verify (its statuses are the caller's); the verdict
// algorithm uploads the columns to the key-set staging area as that call does (one such call at a time per device, host_mu),
// and on a verdict of 0 the statuses come from jjs_keyset_verify.
int jjs_keyset_verify_all(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2,
                          const uint8_t* m, size_t n, uint8_t* status, int* verdict) {
    if (!verdict) return fail(JJS_ERR_ARG, "null verdict");
    device_state* dev = nullptr;
    int scheme = 0;
    bool msm = false;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        keyset_entry* k = find_keyset(ks);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (n == 0) { *verdict = 1; return JJS_OK; }
        if (int rc = keyset_check_cols(k->scheme, format, key_idx, s0, s1, s2, m, false)) return rc;
        scheme = k->scheme;
        msm = keyset_verdict_route(scheme, format, n);
        dev = g;
        if (msm) ++g_keyset_host_calls;       // jjs_shutdown does not free `dev` before this call has left
    }
    uint64_t tally[4] = {};
    if (!msm) {
        if (int rc = jjs_keyset_verify(ks, format, key_idx, s0, s1, s2, m, n, status, tally)) return rc;
        *verdict = tally[0] == n ? 1 : 0;
        return JJS_OK;
    }
    int v = 0;
    {
        struct leave {
            ~leave() {
                std::lock_guard<std::mutex> lock(L.mu);
                --g_keyset_host_calls;
                L.lane_cv.notify_all();
            }
        } leave_on_every_way_out;
        std::lock_guard<std::mutex> big(dev->host_mu);
        g = dev;
        int rc = no_throw([&]() -> int {
            const size_t widths[5] = {4, 32, 64, scheme == JJS_SCHEME_DOUBLE ? (size_t)64 : (size_t)0, 32};      // affine signatures
            const void* src[5] = {key_idx, s0, s1, s2, m};
            size_t off[6], total = 0;
            for (int i = 0; i < 5; ++i) { off[i] = total; total += pad256(widths[i] * n); }
            off[5] = total; total += 256;                             // the verdict word
            if (total > dev->ks_stage_bytes) {
                const size_t cap = grown(total);
                if (int r = regrow(dev->ks_stage, dev->ks_stage_bytes, dev->ks_stage_bytes, cap, cap)) return r;
            }
            HIP_TRY(hipSetDevice(dev->device));
            hipStream_t s = dev->ks_stream;
            const void* d[5] = {};
            for (int i = 0; i < 5; ++i) {
                if (!widths[i]) continue;
                d[i] = dev->ks_stage + off[i];
                HIP_TRY(hipMemcpyAsync(dev->ks_stage + off[i], src[i], widths[i] * n, hipMemcpyHostToDevice, s));
            }
            uint32_t* vw = reinterpret_cast<uint32_t*>(dev->ks_stage + off[5]);
            {
                std::lock_guard<std::mutex> lock(L.mu);
                if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
                keyset_entry* k = find_keyset(ks);
                if (!k) return fail(JJS_ERR_ARG, "the key set was destroyed during the call");
                const keyset_copy* c = keyset_copy_for(*k, dev);
                if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
                if (int r = keyset_verdict_launch_msm(*k, *c, d, n, vw, s)) return r;
            }
            uint32_t hv = 0;
            HIP_TRY(hipMemcpyAsync(&hv, vw, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            v = hv ? 1 : 0;
            return JJS_OK;
        });
        if (rc) return rc;
    }
    *verdict = v;
    if (status) {
        if (v) memset(status, 0, n);
        else if (int rc = jjs_keyset_verify(ks, format, key_idx, s0, s1, s2, m, n, status, tally)) return rc;
    }
    return JJS_OK;
}

}  // extern "C"

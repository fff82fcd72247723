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

// The key points of a call over n items against k (ksv_run_kernel, ksv_key_kernel): their geometry and their parts of the
// verdict scratch, behind the MSM's: the items' scalars, the heads and the cells of the runs per point column, the blocks'
// key points.
struct ksv_key_geometry {
    uint32_t cells, point_blocks;
    size_t extra[7];
};
static ksv_key_geometry ksv_key_parts(const keyset_entry& k, size_t n) {
    ksv_key_geometry G{};
    G.cells = ksv_cells(n);
    G.point_blocks = (uint32_t)(((uint64_t)k.n_cols * k.n_keys + BLOCK - 1) / BLOCK);
    const size_t second = k.n_cols > 1 ? 1 : 0;          // (no second point column: no second scalar column)
    const size_t extra[7] = {n * 32, second * n * 32, (size_t)k.n_keys * 32, second * k.n_keys * 32, (size_t)G.cells * 32, second * G.cells * 32,
                             (size_t)G.point_blocks * MSM_EXT_WORDS * 4};
    for (int i = 0; i < 7; ++i) G.extra[i] = extra[i];
    return G;
}
// ... their descriptor over the front's sort (F), the scalar columns a0 / a1 and the carved parts q[2 .. 6]
static ksv_key_params ksv_key_setup(const keyset_entry& k, const keyset_copy& c, const keyset_front& F, size_t n, const uint8_t* a0,
                                    const uint8_t* a1, uint8_t* const* q) {
    const uint32_t stride = k.n_keys < CURSOR_DENSE_FROM ? CURSOR_STRIDE : 1u;
    ksv_key_params S{};
    S.R = ksv_runs{F.K.key_cursor, stride, F.K.order, F.X.keyid, k.n_keys, n};
    S.n_cols = k.n_cols;
    S.a[0] = a0; S.a[1] = a1;
    for (int i = 0; i < 2; ++i) {
        S.head[i] = q[2 + i]; S.cell[i] = q[4 + i];
        S.key_flags[i] = c.flags[i]; S.tables[i] = c.tables[i];
    }
    S.points = reinterpret_cast<uint32_t*>(q[6]);
    return S;
}
// ... and their launches: the runs' pieces, then S_k * PK_k over the set's tables
static void ksv_key_launch(const keyset_entry& k, const ksv_key_geometry& G, const ksv_key_params& S, hipStream_t s) {
    hipLaunchKernelGGL(ksv_run_kernel, dim3((unsigned)grid_for(8192, (size_t)k.n_cols * (k.n_keys + G.cells))), dim3(BLOCK), 0, s, S);
    hipLaunchKernelGGL(ksv_key_kernel, dim3(G.point_blocks), dim3(BLOCK), 0, s, S);
}

// The front of the verdict algorithm on stream s (under L.mu; g is c's device), up to and including the item pass: the seed,
// the grouping of the items by key, the descriptor over d = key_idx, u, R, R', m (device, affine signatures), the MSM's shape
// (window: its width, 0 = by size), the scratch, the clear, ksv_item_kernel over `blocks` blocks (0: the call's own grid).  It
// returns with the slot shared (begin_shared): the caller queues what reads the scratch and ends with end_shared.
struct keyset_verdict_front {
    ksv_params B;
    msm_params M;
    ksv_key_geometry G;
    ksv_key_params S;
    uint32_t blocks;
    uint32_t* span_sum;
};
static int keyset_verdict_front_launch(keyset_entry& k, const keyset_copy& c, const void* const* d, size_t n, int window, uint32_t blocks,
                                       hipStream_t s, keyset_verdict_front& V) {
    ksv_params& B = V.B;
    msm_params& M = V.M;
    B = ksv_params{};
    if (int rc = batch_seed(B.seed)) return rc;
    keyset_front F;
    if (int rc = keyset_front_end(k, c, d[0], n, true, s, F)) return rc;
    B.V = keyset_params(k.scheme, c, (const uint8_t*)d[1], (const uint8_t*)d[2], (const uint8_t*)d[3], (const uint8_t*)d[4], n,
                        out_ptrs{nullptr, nullptr, nullptr, nullptr});
    B.n_cols = k.n_cols;
    B.keyid = F.X.keyid;
    for (uint32_t i = 0; i < k.n_cols; ++i) B.key_flags[i] = c.flags[i];

    M = msm_params{};
    M.n = n; M.N = (uint64_t)B.V.n_eq * n;
    M.neg_kinds = (1u << B.V.n_eq) - 1u;                 // every term is a -R
    static_cast<msm_shape&>(M) = msm_shape_short(window ? window : msm_window(msm_pick_short_window(M.N)));
    B.z_bits = msm_weight_bits(M.c);
    V.blocks = blocks ? blocks : (uint32_t)grid_for(g->grid_prepare, n);
    const size_t nb = (size_t)M.W * M.B;
    V.G = ksv_key_parts(k, n);
    uint8_t* q[7];
    V.span_sum = nullptr;
    if (int rc = verdict_scratch(B, M, V.blocks, V.G.extra, 7, q, V.span_sum)) return rc;
    B.a[0] = q[0]; B.a[1] = q[1];
    V.S = ksv_key_setup(k, c, F, n, B.a[0], B.a[1], q);

    if (int rc = begin_shared(s)) return rc;
    clear_params Z{};
    Z.p[0] = B.fail; Z.bytes[0] = 4;
    Z.p[1] = M.off; Z.bytes[1] = (nb + 1) * 4;
    Z.p[2] = wire_bad(); Z.bytes[2] = n;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)grid_for(256, (nb > n ? nb : n) / 16 + 1)), dim3(BLOCK), 0, s, Z);
    keyset_front_launch(F, true, s);
    hipLaunchKernelGGL(ksv_item_kernel, dim3(V.blocks), dim3(BLOCK), 0, s, B);
    return JJS_OK;
}
// The verdict algorithm on stream s (under L.mu; g is c's device): d = key_idx, u, R, R', m (device, affine signatures).
static int keyset_verdict_launch_msm(keyset_entry& k, const keyset_copy& c, const void* const* d, size_t n, uint32_t* verdict, hipStream_t s) {
    keyset_verdict_front V;
    if (int rc = keyset_verdict_front_launch(k, c, d, n, 0, 0, s, V)) return rc;
    ksv_key_launch(k, V.G, V.S, s);
    msm_launch(V.M, V.span_sum, s);                      // over the R terms
    hipLaunchKernelGGL(ksv_final_kernel, dim3(1), dim3(BLOCK), 0, s, V.B, V.M, V.blocks, (const uint32_t*)V.S.points, V.G.point_blocks, verdict);
    HIP_TRY(hipGetLastError());
    return end_shared(s);
}
// The per-item route on stream s (under L.mu): the key-set call with its tally in the slot, then the verdict from the tally.
static int keyset_verdict_launch_items(keyset_entry& k, const keyset_copy& c, int format, const void* const* d, size_t n, uint32_t* verdict,
                                       hipStream_t s) {
    pick_slot(n, s);
    if (int rc = sl->verdict.ensure(256)) return rc;
    unsigned long long* tally = reinterpret_cast<unsigned long long*>(sl->verdict.get());
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
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    hipStream_t s = (hipStream_t)stream;
    if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
    if (int rc = verdict_word_dev(verdict, n, s)) return rc;
    if (n == 0) return JJS_OK;
    if (int rc = keyset_check_cols(k->scheme, format, key_idx, s0, s1, s2, m, true)) return rc;
    const keyset_copy* c = copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    const void* d[] = {key_idx, s0, s1, s2, m};
    return no_throw([&] {
        return keyset_verdict_route(k->scheme, format, n) ? keyset_verdict_launch_msm(*k, *c, d, n, (uint32_t*)verdict, s)
                                                          : keyset_verdict_launch_items(*k, *c, format, d, n, (uint32_t*)verdict, s);
    });
}

// A host-buffer verdict call: blocking.  The per-item route is jjs_keyset_verify (its statuses are the caller's); the verdict
// algorithm's is verdict_host_msm (verdict_calls.h).
int jjs_keyset_verify_all(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2,
                          const uint8_t* m, size_t n, uint8_t* status, int* verdict) {
    if (!verdict) return fail(JJS_ERR_ARG, "null verdict");
    device_state* dev = nullptr;
    int scheme = 0;
    bool msm = false;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (n == 0) { *verdict = 1; return JJS_OK; }
        if (int rc = keyset_check_cols(k->scheme, format, key_idx, s0, s1, s2, m, false)) return rc;
        scheme = k->scheme;
        msm = keyset_verdict_route(scheme, format, n);
        dev = g;
        if (msm) ++g_blocking_calls;       // jjs_shutdown does not free `dev` before this call has left
    }
    uint64_t tally[4] = {};
    auto per_item = [&] { return jjs_keyset_verify(ks, format, key_idx, s0, s1, s2, m, n, status, tally); };
    if (!msm) {
        if (int rc = per_item()) return rc;
        *verdict = tally[0] == n ? 1 : 0;
        return JJS_OK;
    }
    const size_t widths[5] = {4, 32, 64, scheme == JJS_SCHEME_DOUBLE ? (size_t)64 : (size_t)0, 32};      // affine signatures
    const void* src[5] = {key_idx, s0, s1, s2, m};
    return verdict_host_msm(dev, &ks, widths, src, 5, n,
                            [&](keyset_entry* k, const keyset_copy* c, const void* const* d, uint32_t* vw, hipStream_t s) {
                                return keyset_verdict_launch_msm(*k, *c, d, n, vw, s);
                            },
                            per_item, status, verdict);
}

#if defined(JJS_PROFILING)
// include/jjs_gpu_profiling.h: the item pass of a key-set verdict call -- keyset_verdict_front_launch, as
// keyset_verdict_launch_msm runs it -- with what it wrote copied out
int jjs_debug_keyset_items_dev(jjs_keyset ks, const void* key_idx, const void* u, const void* R, const void* Rp, const void* m, size_t n, int c,
                               unsigned blocks, void* scalars_out, void* a0_out, void* a1_out, void* partial_out, void* fail_out, void* zu_out,
                               unsigned* blocks_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (int rc = debug_items_args(n, 2ull * n, c, blocks, scalars_out, partial_out, fail_out, zu_out, blocks_out)) return rc;
    if (!all_ok(a0_out) || (k->n_cols > 1 && !all_ok(a1_out))) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    if (int rc = keyset_check_cols(k->scheme, JJS_FORMAT_AFFINE, key_idx, u, R, Rp, m, true)) return rc;
    const keyset_copy* cp = copy_for(*k, g);
    if (!cp) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    const void* d[] = {key_idx, u, R, Rp, m};
    hipStream_t s = (hipStream_t)stream;
    return no_throw([&]() -> int {
        keyset_verdict_front V;
        if (int rc = keyset_verdict_front_launch(*k, *cp, d, n, c, blocks, s, V)) return rc;
        *blocks_out = V.blocks;
        int rc = debug_items_out(V.B.scalars, (size_t)V.M.N * 32, V.B.partial, V.blocks, V.B.fail, scalars_out, partial_out, fail_out, zu_out, s);
        if (!rc && hipMemcpyAsync(a0_out, V.B.a[0], n * 32, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = fail(JJS_ERR_HIP, "copying the scalar column");
        if (!rc && k->n_cols > 1 && hipMemcpyAsync(a1_out, V.B.a[1], n * 32, hipMemcpyDeviceToDevice, s) != hipSuccess)
            rc = fail(JJS_ERR_HIP, "copying the scalar column");
        const int rc2 = end_shared(s);
        return rc ? rc : rc2;
    });
}
// include/jjs_gpu_profiling.h: the run sums and the key points of keyset_verdict_launch_msm under the caller's own scalar
// columns -- the same front end, scratch, descriptor and launches, then dbg_ksv_sums_kernel
int jjs_debug_keyset_sums_dev(jjs_keyset ks, const void* key_idx, const void* a0, const void* a1, size_t n, void* sums_out, void* point_out,
                              void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (n == 0 || n >= 0x80000000ull) return fail(JJS_ERR_ARG, "the item count is out of range");
    if (!all_ok(key_idx, a0, sums_out, point_out) || (k->n_cols > 1 && !all_ok(a1))) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    const keyset_copy* c = copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    hipStream_t s = (hipStream_t)stream;
    return no_throw([&]() -> int {
        keyset_front F;
        if (int rc = keyset_front_end(*k, *c, key_idx, n, true, s, F)) return rc;
        ksv_params B{};
        msm_params M{};                                      // no terms: the smallest shape
        M.n = n;
        static_cast<msm_shape&>(M) = msm_shape_short(8);
        const ksv_key_geometry G = ksv_key_parts(*k, n);
        uint8_t* q[7];
        uint32_t* span_sum = nullptr;
        if (int rc = verdict_scratch(B, M, 1, G.extra, 7, q, span_sum)) return rc;
        const ksv_key_params S = ksv_key_setup(*k, *c, F, n, (const uint8_t*)a0, (const uint8_t*)a1, q);
        if (int rc = begin_shared(s)) return rc;
        clear_params Z{};
        Z.p[2] = wire_bad(); Z.bytes[2] = n;
        hipLaunchKernelGGL(clear_kernel, dim3((unsigned)grid_for(256, n / 16 + 1)), dim3(BLOCK), 0, s, Z);
        keyset_front_launch(F, true, s);
        ksv_key_launch(*k, G, S, s);
        hipLaunchKernelGGL(dbg_ksv_sums_kernel, dim3(G.point_blocks), dim3(BLOCK), 0, s, S, G.point_blocks, (uint8_t*)sums_out, (uint32_t*)point_out);
        HIP_TRY(hipGetLastError());
        return end_shared(s);
    });
}
#endif

}  // extern "C"

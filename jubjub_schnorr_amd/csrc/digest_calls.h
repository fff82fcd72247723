// Part of jjs_gpu.hip (included among the extern "C" entry points, behind the signers): jjs_digest(_dev) -- Poseidon digests of
// ragged inputs (digest.h, include/jjs_gpu.h) -- and jjs_debug_digest_limits.
//
// A call is routed as a whole, by n alone: at most DIGEST_COOP_MAX_ITEMS items take eight lanes each (digest_coop_kernel), more
// take one (digest_kernel), in a grid of at most the lanes resident at once.  A uniform call (offsets NULL) uploads nothing, and
// uses no scratch unless its length lies beyond the tag table (digest_tags_kernel then writes its one tag there).  A ragged call
// uploads its offsets and the order of its items (dg_block_order) into the device's digest scratch (device_state::digest_scratch,
// grow-only by grown.h's rule, used in the order of slot 0's event as the signers' tables are), where the tags of its long items
// go too; the order is formed in host memory the device keeps for it (digest_order), so that no call allocates once both have
// reached its shape.

// The crossover of the two routes, by record (profiles/r22_digest.jsonl, variant c: the two routes forced in turn in the profiling
// build, ms per call, eight lanes against one, medians of 5 rounds).  8 192 items is the largest recorded n at which eight lanes per
// item win at both lengths beyond the spreads -- k = 5: 0.305 against 0.461, k = 64: 2.07 against 3.50, as at every smaller n
// (0.55-0.66x).  At 16 384 they are level at k = 5 (0.461 / 0.462) and 0.95x at k = 64 (3.34 / 3.51); from 32 768 on they take
// 1.7-4.2x the time.  8 192 is also MSIG_COOP_MAX_ITEMS, for the reason given there: up to it eight lanes per item leave the device
// at most a wave per SIMD.  No n between 8 192 and 16 384 was recorded.
constexpr size_t DIGEST_COOP_MAX_ITEMS = 8192;
#if defined(JJS_PROFILING)
static int g_force_digest_route = 0;         // jjs_debug_force_path 0x1000000: the coop route at any n; 0x2000000: the lane route
static bool g_digest_keep_order = false;     // ... 0x4000000: a ragged call's lanes take the items in input order
#endif

extern "C++" {
struct digest_call {
    int format, flags;
    const void* in;
    const uint32_t* offsets;                 // host memory; null: every item has k elements
    size_t k, n;
    void *out, *status;
};
static size_t digest_width(int format) { return format == JJS_DIGEST_WIDE ? 64 : 32; }
// What every form checks (n > 0): format and flags, the lengths, the pointers.  `elements`: the elements of the call; `any_long`:
// an item lies beyond the tag table.
static int digest_args(const digest_call& A, bool device, size_t& elements, bool& any_long) {
    if (A.format != JJS_DIGEST_CANONICAL && A.format != JJS_DIGEST_WIDE) return fail(JJS_ERR_ARG, "format out of range");
    if (A.flags & ~JJS_DIGEST_TRUNCATED) return fail(JJS_ERR_ARG, "flags: only bit 0 (JJS_DIGEST_TRUNCATED) is defined");
    if (A.n > 0xffffffffull) return fail(JJS_ERR_ARG, "a call digests at most 2^32 - 1 items");
    if (A.offsets) {
        if (A.offsets[0] != 0) return fail(JJS_ERR_ARG, "offsets must start at 0");
        for (size_t i = 0; i < A.n; ++i) {
            if (A.offsets[i + 1] < A.offsets[i]) return fail(JJS_ERR_ARG, "item %zu: offsets must not decrease", i);
            const uint32_t len = A.offsets[i + 1] - A.offsets[i];
            if (len == 0) return fail(JJS_ERR_ARG, "item %zu is empty: the digest of no elements is not defined here", i);
            if (len > DG_MAX_LEN) return fail(JJS_ERR_ARG, "item %zu: %u elements (the SAFE tag encodes at most 2^31 - 1)", i, (unsigned)len);
            any_long = any_long || len >= DG_TABLE_TAGS;
        }
        elements = A.offsets[A.n];
    } else {
        if (A.k == 0) return fail(JJS_ERR_ARG, "k = 0: the digest of no elements is not defined here");
        if (A.k > DG_MAX_LEN) return fail(JJS_ERR_ARG, "k = %zu (the SAFE tag encodes at most 2^31 - 1)", A.k);
        if (A.n > SIZE_MAX / 64 / A.k) return fail(JJS_ERR_ARG, "n * k overflows");
        elements = A.n * A.k;
        any_long = A.k >= DG_TABLE_TAGS;
    }
    if (!A.in || !A.out) return fail(JJS_ERR_ARG, "null column");
    if (device && (!aligned16(A.in) || !aligned16(A.out))) return fail(JJS_ERR_ARG, "misaligned column");
    return JJS_OK;
}
static bool digest_coop_route(size_t n) {
#if defined(JJS_PROFILING)
    if (g_force_digest_route) return g_force_digest_route == 1;
#endif
    return n <= DIGEST_COOP_MAX_ITEMS;
}
// The call on device columns, queued on st (under the engine's mutex, g the device; n > 0, the arguments checked).
static int digest_locked(const digest_call& A, bool any_long, hipStream_t st) {
    const size_t n = A.n;
    const bool ragged = A.offsets != nullptr;
    digest_params D{};
    D.in = (const uint8_t*)A.in; D.out = (uint8_t*)A.out; D.status = (uint8_t*)A.status;
    D.tags = g->tags_long; D.n = n; D.k = (uint32_t)A.k; D.flags = (uint32_t)A.flags;
    const bool coop = digest_coop_route(n);
    const dim3 grid((unsigned)grid_for(g->grid_digest, coop ? n * DG_COOP_LANES : n));
    auto launch = [&]() -> int {
        if (any_long) hipLaunchKernelGGL(digest_tags_kernel, dim3((unsigned)grid_for(4096, ragged ? n : 1)), dim3(BLOCK), 0, st, D);
        if (coop) {
            if (A.format == JJS_DIGEST_WIDE) hipLaunchKernelGGL(digest_coop_kernel<DG_WIDE>, grid, dim3(BLOCK), 0, st, D);
            else hipLaunchKernelGGL(digest_coop_kernel<DG_CANONICAL>, grid, dim3(BLOCK), 0, st, D);
        } else {
            if (A.format == JJS_DIGEST_WIDE) hipLaunchKernelGGL(digest_kernel<DG_WIDE>, grid, dim3(BLOCK), 0, st, D);
            else hipLaunchKernelGGL(digest_kernel<DG_CANONICAL>, grid, dim3(BLOCK), 0, st, D);
        }
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    };
    if (!ragged && !any_long) return launch();
    // the scratch: [offsets, n + 1 words | order, n words] of a ragged call, then the tags of a call with an item beyond the table (9
    // words per item, or 9 for a uniform call); the order is formed in the device's host words [order | tmp]
    const size_t off_bytes = ragged ? pad256((n + 1) * sizeof(uint32_t)) : 0, order_bytes = ragged ? pad256(n * sizeof(uint32_t)) : 0;
    const size_t tag_bytes = any_long ? 9 * sizeof(uint32_t) * (ragged ? n : 1) : 0;
    if (int rc = g->digest_scratch.ensure(off_bytes + order_bytes + tag_bytes)) return rc;
    if (ragged) {
        if (g->digest_order.size() < 2 * n) g->digest_order.resize(grown(2 * n));
        dg_block_order(A.offsets, n, g->digest_order.data() + n, g->digest_order.data());
    }
    big_slot();
    if (int rc = begin_shared(st)) return rc;
    auto queue = [&]() -> int {
        uint8_t* base = g->digest_scratch.get();
        if (ragged) {
            HIP_TRY(hipMemcpyAsync(base, A.offsets, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            D.offsets = reinterpret_cast<const uint32_t*>(base);
            bool ordered = true;
#if defined(JJS_PROFILING)
            ordered = !g_digest_keep_order;
#endif
            if (ordered) {
                // (a pageable source: staged by the runtime before the call returns, so the next call may rewrite digest_order)
                HIP_TRY(hipMemcpyAsync(base + off_bytes, g->digest_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                D.order = reinterpret_cast<const uint32_t*>(base + off_bytes);
            }
        }
        if (any_long) {
            D.long_tags = reinterpret_cast<uint32_t*>(base + off_bytes + order_bytes);
            D.long_stride = ragged ? 9u : 0u;
        }
        return launch();
    };
    const int rc = queue();
    const int rc2 = end_shared(st);             // the slot's event covers whatever was queued, also when a step failed
    return rc ? rc : rc2;
}
}  // extern "C++"

extern "C" {

int jjs_digest_dev(int format, int flags, const void* in, const uint32_t* offsets_host, size_t k, size_t n, void* out, void* status,
                   void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    const digest_call A{format, flags, in, offsets_host, k, n, out, status};
    size_t elements = 0;
    bool any_long = false;
    if (int rc = digest_args(A, true, elements, any_long)) return rc;
    return no_throw([&] { return digest_locked(A, any_long, (hipStream_t)stream); });
}

// From host buffers, blocking, on the frame of staged_host_call.h.  parts: the elements in; the digests and the statuses out (a
// status column the caller does not ask for is not staged, and the kernels write none).
int jjs_digest(int format, int flags, const uint8_t* in, const uint32_t* offsets, size_t k, size_t n, uint8_t* out, uint8_t* status) {
    const digest_call H{format, flags, in, offsets, k, n, out, status};
    size_t elements = 0;
    bool any_long = false;
    return staged_host_call(
        [&](bool& go) -> int {
            if (n == 0) return JJS_OK;
            go = true;
            return digest_args(H, false, elements, any_long);
        },
        [&] {
            return std::vector<stage_part>{{elements * digest_width(format), in, nullptr}, {n * 32, nullptr, out}, {status ? n : 0, nullptr, status}};
        },
        [&](uint8_t* const* p, hipStream_t st) {
            digest_call A = H;
            A.in = p[0]; A.out = p[1]; A.status = status ? p[2] : nullptr;
            return digest_locked(A, any_long, st);
        });
}

// [0] the largest n the eight-lanes-per-item route serves, [1] the lanes of digest_kernel's grid on the current device (its grid
// limit times the block size: a call of more items takes a second trip through the grid-stride loop).
int jjs_debug_digest_limits(uint64_t out[2]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    out[0] = (uint64_t)DIGEST_COOP_MAX_ITEMS;
    out[1] = (uint64_t)g->grid_digest * BLOCK;
    return JJS_OK;
}

}  // extern "C"

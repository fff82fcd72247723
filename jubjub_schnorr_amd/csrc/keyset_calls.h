// Part of jjs_gpu.hip (included among the extern "C" entry points): registered key sets (keyset.h, include/jjs_gpu.h
// jjs_keyset_*) -- building a set on every driven device, the registry, and the calls against a set.

extern "C++" {        // (templates below)
// One jjs_*_create call, from its first section under L.mu to the published handle.  The object is built outside the engine's
// mutex, on a stream of its own per device (other threads' calls go on meanwhile), and published in its registry under the
// mutex once every copy is complete.  While it is being built the call counts among the blocking calls jjs_shutdown waits
// for, so the devices it uses stay alive.  Nothing here throws.
// The three steps are called in this order, each only after the one before returned JJS_OK (`e` is null until enter() has).
template <class Entry>
class registration {
    std::vector<device_state*> devs;       // the devices the engine drove when the call came in
    std::optional<blocking_call_leave> leave_on_every_way_out;
    void free_copies() { e->copies.clear(); }     // nothing has been published, and each copy's build stream was drained: freed, not retired
public:
    std::unique_ptr<Entry> e;              // the entry, from enter() until it is published
    // the first section under L.mu: the engine is ready, check() accepts the arguments; then the call is counted in
    template <class Check>
    int enter(Check check) {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        if (int rc = check()) return rc;
        if (int rc = no_throw([&] { devs = L.devs; e.reset(new Entry()); return JJS_OK; })) return rc;
        ++g_blocking_calls;
        leave_on_every_way_out.emplace();
        return JJS_OK;
    }
    // build_copy(copy, stream) on every device in turn (g is that device), each on a non-blocking stream of its own
    template <class BuildCopy>
    int build(BuildCopy build_copy) {
        device_restore restore;
        const int rc = no_throw([&]() -> int {
            for (device_state* d : devs) {
                g = d;
                HIP_TRY(hipSetDevice(d->device));
                stream_owner s;
                HIP_TRY(s.create(hipStreamNonBlocking));
                e->copies.emplace_back();
                if (int brc = build_copy(e->copies.back(), s)) { e->copies.pop_back(); return brc; }
            }
            return JJS_OK;
        });
        if (rc) free_copies();
        return rc;
    }
    // the second section under L.mu: the engine still drives the same devices; the entry goes into `reg`, its handle to *out
    int publish(registry<Entry>& reg, const char* what, uint64_t* out) {
        std::lock_guard<std::mutex> lock(L.mu);
        int rc = L.devs != devs ? fail(JJS_ERR_NOT_INIT, "the engine's devices changed while the %s was built", what)
                                : no_throw([&] { *out = reg.publish(e); return JJS_OK; });
        if (rc) free_copies();
        return rc;
    }
};
// The frame of one device's copy `c` of an object (g is that device; `what`: the object, for the messages): the copy's own
// allocation of `bytes`, a build area of `tmp_bytes` beside it, body(build area), which carves both and queues the build on
// stream s; then the stream is drained and the build area freed -- and the copy with it when the body failed.
template <class Body>
static int build_device_copy(device_copy& c, size_t bytes, size_t tmp_bytes, const char* what, hipStream_t s, Body body) {
    c.dev = g;
    if (c.mem.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(JJS_ERR_HIP, "hipMalloc of a %s (%zu bytes) failed", what, bytes);
    }
    device_mem<uint8_t> tmp;
    if (tmp.alloc(tmp_bytes) != hipSuccess) {
        (void)hipGetLastError();
        (void)c.mem.free();
        return fail(JJS_ERR_HIP, "hipMalloc of a %s's build area (%zu bytes) failed", what, tmp_bytes);
    }
    const int rc = body(tmp.get());
    (void)hipStreamSynchronize(s);        // ... so that the build area may go, and the copy with it when the body failed
    if (rc) (void)c.mem.free();
    return rc;
}
}  // extern "C++"

static uint32_t keyset_cols(int scheme) { return scheme == JJS_SCHEME_SINGLE ? 1u : 2u; }

// the lookup table of a set's copy as its kernels take it
static keyset_lookup keyset_lookup_of(const keyset_entry& k, const keyset_copy& c) {
    keyset_lookup T{};
    for (uint32_t i = 0; i < k.n_cols; ++i) { T.keys[i] = c.keys[i]; T.flags[i] = c.flags[i]; }
    T.on_curve = c.on_curve; T.slots = c.lookup; T.mask = c.lookup_mask;
    T.n_keys = k.n_keys; T.n_cols = k.n_cols; T.seed = k.lookup_seed;
    return T;
}

// One device's copy of a set (g is that device): the keys uploaded and decoded / normalised into the copy, their flags, the
// chains of bases (freed with the upload area) and the window tables of the valid keys -- the key-table path's own kernels
// with a key_params whose "distinct keys" are the set's keys in order.  `flags_out` receives the flags of every point column.
static int keyset_build_copy(keyset_entry& k, keyset_copy& c, int format, const uint8_t* keys, const uint8_t* keys2,
                             std::vector<uint8_t>& flags_out, hipStream_t s) {
    const uint32_t n = k.n_keys, cols = k.n_cols;
    const int w = KEYSET_WINDOW;
    const size_t key_bytes = pad256((size_t)n * 64), flag_bytes = pad256(n);
    const size_t table_bytes = (size_t)n * kt_positions(w) * kt_table_words(w) * 4;
    const uint32_t lookup_slots = kl_slot_count(n);
    const size_t lookup_bytes = pad256((size_t)lookup_slots * 4);
    // the build area: the uploaded encodings, the chains of bases, key_item, the valid-key lists, the malformed flags
    const size_t in_width = format == JJS_FORMAT_EXT ? 96 : (format == JJS_FORMAT_WIRE ? 32 : 0);
    const size_t in_bytes = pad256((size_t)n * in_width * cols), base_bytes = pad256((size_t)n * kt_positions(w) * KT_BASE_WORDS * 4);
    const size_t item_bytes = pad256((size_t)n * 4), valid_bytes = pad256(((size_t)n + 1) * 4), scratch_bytes = pad256((size_t)n * 48);
    const size_t tmp_bytes = in_bytes + cols * (base_bytes + valid_bytes) + item_bytes + flag_bytes + scratch_bytes;
    // host memory the queued copies read or write: it outlives the frame, which drains the stream on every way out
    std::vector<uint32_t> host(64 > n ? 64 : n);
    for (uint32_t i = 0; i < n; ++i) host[i] = i;
    uint32_t words[64] = {n, n, (uint32_t)w};
    flags_out.assign((size_t)cols * n, 0);
    return build_device_copy(c, 256 + cols * (key_bytes + flag_bytes + pad256(table_bytes)) + lookup_bytes + flag_bytes, tmp_bytes, "key set", s, [&](uint8_t* tmp) -> int {
        uint8_t* p = c.mem;
        c.words = reinterpret_cast<uint32_t*>(p); p += 256;
        for (uint32_t i = 0; i < cols; ++i) {
            c.keys[i] = p; p += key_bytes;
            c.flags[i] = p; p += flag_bytes;
            c.tables[i] = reinterpret_cast<uint32_t*>(p); p += pad256(table_bytes);
        }
        c.lookup = reinterpret_cast<uint32_t*>(p); p += lookup_bytes;
        c.lookup_mask = lookup_slots - 1;
        c.on_curve = p; p += flag_bytes;
        uint8_t* q = tmp;
        uint8_t* in = q; q += in_bytes;
        uint32_t* key_item = reinterpret_cast<uint32_t*>(q); q += item_bytes;
        uint8_t* bad = q; q += flag_bytes;
        uint32_t* scratch = reinterpret_cast<uint32_t*>(q); q += scratch_bytes;
        key_params K{};
        K.n_cols = cols; K.max_keys = n; K.max_keys_wide = n; K.quad_chains = 1; K.n = n; K.counters = c.words;
        for (uint32_t i = 0; i < cols; ++i) {
            key_column& C = K.col[i];
            C.src = fe_src{c.keys[i], 64, 0};
            C.key_item = key_item;
            C.key_flags = c.flags[i];
            C.bases = reinterpret_cast<uint32_t*>(q); q += base_bytes;
            C.valid_ids = reinterpret_cast<uint32_t*>(q); q += valid_bytes;
            C.tables = c.tables[i];
        }
        HIP_TRY(hipMemcpyAsync(key_item, host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c.words, words, sizeof(words), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(bad, 0, flag_bytes, s));
        for (uint32_t i = 0; i < cols; ++i) HIP_TRY(hipMemsetAsync(c.tables[i], 0, table_bytes, s));   // invalid keys get no tables
        const uint8_t* src[2] = {keys, keys2};
        if (format == JJS_FORMAT_AFFINE) {
            for (uint32_t i = 0; i < cols; ++i) HIP_TRY(hipMemcpyAsync(c.keys[i], src[i], (size_t)n * 64, hipMemcpyHostToDevice, s));
        } else if (format == JJS_FORMAT_EXT) {
            normalize_params N{};
            for (uint32_t i = 0; i < cols; ++i) {
                HIP_TRY(hipMemcpyAsync(in + (size_t)i * n * 96, src[i], (size_t)n * 96, hipMemcpyHostToDevice, s));
                N.src[i] = fe_src{in + (size_t)i * n * 96, 96, 0};
                N.out[i] = c.keys[i];
            }
            N.n_src = cols; N.bad = bad; N.scratch = scratch;
            if (int e = launch_normalize(N, 0, n, n, s)) return e;
        } else {
            HIP_TRY(hipMemcpyAsync(in, keys, (size_t)n * 32 * cols, hipMemcpyHostToDevice, s));     // n x 32, or n x (pk || pk')
            decode_params D{};
            D.n_src = cols; D.n = n; D.bad = bad;
            for (uint32_t i = 0; i < cols; ++i) { D.src[i] = fe_src{in, 32 * cols, 32 * i}; D.out[i] = c.keys[i]; }
            D.dlog = dlog_tables{g->dlog_pow, g->dlog_hash};
            hipLaunchKernelGGL(decode_kernel, dim3((unsigned)grid_for(8192, n)), dim3(BLOCK), 0, s, D);
        }
        hipLaunchKernelGGL(key_chain_kernel, dim3((unsigned)((5ull * cols * n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, K);
        hipLaunchKernelGGL(keyset_flags_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, c.flags[0], cols > 1 ? c.flags[1] : nullptr,
                           (const uint8_t*)bad, n);
        hipLaunchKernelGGL(key_table_kernel, dim3((unsigned)(((uint64_t)cols * n * KT_MAX_POSITIONS + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, K);
        // the lookup table of the by-key calls (keyset_lookup.h), behind the flags it reads: part of the set before it is published
        HIP_TRY(hipMemsetAsync(c.lookup, 0xFF, (size_t)lookup_slots * 4, s));
        hipLaunchKernelGGL(keyset_lookup_insert_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, keyset_lookup_of(k, c));
        HIP_TRY(hipGetLastError());
        for (uint32_t i = 0; i < cols; ++i)
            HIP_TRY(hipMemcpyAsync(flags_out.data() + (size_t)i * n, c.flags[i], n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    });
}

// The front of a call against a set's copy `c` on stream s (g is c's device), shared by keyset_launch and
// keyset_verdict_launch_msm: the call's slot, the items' key indices, the sort's order and cursors carved from sl->keys, the
// key descriptor over the set's keys in order, the index pass that gathers the keys per item into wire_pts(2) (3), and the
// verification descriptor over those columns.  Without `sort` the cursors are neither cleared nor used.
struct keyset_front {
    key_params K;
    keyset_index_params X;
    size_t cursor_words;
};
static int keyset_front_end(const keyset_entry& k, const keyset_copy& c, const void* key_idx, size_t n, bool sort, hipStream_t s, keyset_front& F) {
    pick_slot(n, s);
    if (int rc = sl->wire.ensure(n)) return rc;
    F.cursor_words = (size_t)k.n_keys + 1 > (size_t)CURSOR_DENSE_FROM * CURSOR_STRIDE ? (size_t)k.n_keys + 1
                                                                                      : (size_t)CURSOR_DENSE_FROM * CURSOR_STRIDE;
    if (int rc = sl->keys.ensure(2 * pad256(n * 4) + pad256(F.cursor_words * 4))) return rc;
    key_params& K = F.K;
    K = key_params{};
    K.n_cols = k.n_cols; K.max_keys = k.n_keys; K.max_keys_wide = k.n_keys; K.n = n; K.counters = c.words;
    uint8_t* q = sl->keys;
    uint32_t* keyid = reinterpret_cast<uint32_t*>(q); q += pad256(n * 4);
    K.order = reinterpret_cast<uint32_t*>(q); q += pad256(n * 4);
    K.key_cursor = reinterpret_cast<uint32_t*>(q);
    for (uint32_t i = 0; i < k.n_cols; ++i) {
        K.col[i].src = fe_src{c.keys[i], 64, 0};
        K.col[i].keyid = keyid; K.col[i].key_flags = c.flags[i]; K.col[i].tables = c.tables[i];
    }
    keyset_index_params& X = F.X;
    X = keyset_index_params{};
    X.key_idx = (const uint32_t*)key_idx; X.n_keys = k.n_keys; X.n_cols = k.n_cols;
    X.keys[0] = c.keys[0]; X.keys[1] = c.keys[1]; X.out[0] = wire_pts(2); X.out[1] = wire_pts(3);
    X.keyid = keyid; X.bad = wire_bad(); X.n = n;
    X.cursor = sort ? K.key_cursor : nullptr; X.cursor_words = sort ? F.cursor_words : 0;
    return JJS_OK;
}
static verify_params keyset_params(int scheme, const keyset_copy& c, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m,
                                   size_t n, const out_ptrs& o) {
    verify_params P = scheme_params(scheme, u, R, Rp, wire_pts(2), wire_pts(3), m, n, o);
    P.pre_malformed = wire_bad();
    P.key_flag = c.words + 2;
    return P;
}
// the index pass, and with `sort` the counting sort of the items by key
static void keyset_front_launch(const keyset_front& F, bool sort, hipStream_t s) {
    const size_t n = F.K.n;
    hipLaunchKernelGGL(keyset_index_kernel, dim3((unsigned)grid_for(8192, n > F.cursor_words ? n : F.cursor_words)), dim3(BLOCK), 0, s, F.X);
    if (!sort) return;
    const unsigned item_blocks = (unsigned)grid_for(8192, n);
    hipLaunchKernelGGL(key_count_kernel, dim3(item_blocks), dim3(BLOCK), 0, s, F.K);
    hipLaunchKernelGGL(key_scan_kernel, dim3(1), dim3(1024), 0, s, F.K);
    hipLaunchKernelGGL(key_scatter_kernel, dim3(item_blocks), dim3(BLOCK), 0, s, F.K);
}

// The key columns of a by-key call (jjs_keyset_find*, jjs_keyset_verify_keys*) in the call's format: affine or extended
// K0, K1 (K1 null for a set of one point column), wire K0 alone.  Bytes per item of either column (0: not used):
struct keyset_by_key {
    const void *K0, *K1;
    void* idx_out;            // nullable: the caller's copy of the indices
};
static void keyset_key_widths(uint32_t cols, int format, size_t w[2]) {
    if (format == JJS_FORMAT_WIRE) { w[0] = 32 * cols; w[1] = 0; return; }
    w[0] = format == JJS_FORMAT_EXT ? 96 : 64;
    w[1] = cols > 1 ? w[0] : 0;
}
static int keyset_check_key_cols(uint32_t cols, int format, const void* K0, const void* K1, bool device) {
    if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
    size_t w[2];
    keyset_key_widths(cols, format, w);
    if (!K0 || (device && !aligned16(K0))) return fail(JJS_ERR_ARG, "null or misaligned key column");
    if (w[1] && (!K1 || (device && !aligned16(K1)))) return fail(JJS_ERR_ARG, "null or misaligned second key column");
    return JJS_OK;
}
// The probe of n items on stream s: `found` and `idx_out` (either nullable) receive the index of every item's key or KL_MISS.
// Extended keys are normalised first, into wire_pts(2) (3) of the call's slot (the caller has picked it, sized its wire area
// and ordered the stream behind the slot's previous user), in poison mode: an unusable point (U, V or Z >= q, Z = 0) becomes
// 64 bytes of 0xFF, which no entered key has.
static int keyset_probe_launch(const keyset_entry& k, const keyset_copy& c, int format, const keyset_by_key& B, size_t n, uint32_t* found,
                               hipStream_t s) {
    keyset_probe_params Q{};
    Q.T = keyset_lookup_of(k, c);
    Q.K[0] = (const uint8_t*)B.K0; Q.K[1] = (const uint8_t*)B.K1;
    Q.wire = format == JJS_FORMAT_WIRE ? 1u : 0u;
    Q.n = n; Q.found = found; Q.idx_out = (uint32_t*)B.idx_out;
    if (format == JJS_FORMAT_EXT) {
        normalize_params N{};
        N.n_src = k.n_cols; N.poison = 1;
        N.src[0] = fe_src{(const uint8_t*)B.K0, 96, 0}; N.out[0] = wire_pts(2);
        N.src[1] = fe_src{(const uint8_t*)B.K1, 96, 0}; N.out[1] = wire_pts(3);
        N.scratch = wire_scratch(1);
        if (int rc = launch_normalize(N, 0, n, n, s)) return rc;
        Q.K[0] = wire_pts(2); Q.K[1] = wire_pts(3);
    }
    hipLaunchKernelGGL(keyset_probe_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, Q);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
// jjs_keyset_find_dev's launches (g is c's device): only extended keys need a slot.
static int keyset_find_launch(const keyset_entry& k, const keyset_copy& c, int format, const keyset_by_key& B, size_t n, hipStream_t s) {
    if (format != JJS_FORMAT_EXT) return keyset_probe_launch(k, c, format, B, n, nullptr, s);
    pick_slot(n, s);
    if (int rc = sl->wire.ensure(n)) return rc;
    if (int rc = begin_shared(s)) return rc;
    if (int rc = keyset_probe_launch(k, c, format, B, n, nullptr, s)) return rc;
    return end_shared(s);
}

// The launches of one call against a set's copy `c` on stream s (g is c's device).  d = key_idx, s0, s1, s2, m (device).
// A by-key call (B non-null; d[0] is not read) probes the set's lookup table for its indices in front of the index pass, which
// runs a miss as it runs an index beyond the set -- with a stand-in, so that no lane addresses the set for it -- and turns
// the status of every miss into KL_STATUS_NOT_IN_SET behind the last kernel (keyset_miss_kernel).
static int keyset_launch(keyset_entry& k, const keyset_copy& c, int format, const void* const* d, size_t n, void* status, void* tally,
                         hipStream_t s, const keyset_by_key* B = nullptr) {
    const int scheme = k.scheme;
    const bool small = n <= KEYSET_SMALL_MAX_ITEMS;
    keyset_front F;
    if (int rc = keyset_front_end(k, c, d[0], n, !small, s, F)) return rc;
    if (B) {
        if (int rc = sl->found.ensure(n)) return rc;
        F.X.key_idx = sl->found;
    }
    const auto finish = [&]() -> int {
        if (B && !k.removed_from)
            hipLaunchKernelGGL(keyset_miss_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, (const uint32_t*)sl->found.get(),
                               (uint64_t)n, (uint8_t*)status, (unsigned long long*)tally);
        else if (B)         // a set that has been removed from (keyset_remove.h): a key removed under the call is a miss, never status 3
            hipLaunchKernelGGL(keyset_miss_removed_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                               (const uint32_t*)sl->found.get(), (uint64_t)n, (uint8_t*)status, (unsigned long long*)tally, k.n_keys,
                               (const uint8_t*)c.flags[0]);
        HIP_TRY(hipGetLastError());
        return end_shared(s);
    };
    const key_params& K = F.K;
    if (int rc = sl->prep.ensure(n)) return rc;
    if (int rc = sl->pending.ensure(n)) return rc;
    if (small)
        if (int rc = sl->small.ensure(2 * n + 64)) return rc;      // the subgroup tests of the R points (keyset_hash_kernel)
    // the verification descriptor: R (R') as the format gives them, the keys gathered per item into wire_pts(2) (3)
    const uint8_t *R = (const uint8_t*)d[2], *Rp = (const uint8_t*)d[3];
    const uint32_t n_r = scheme == JJS_SCHEME_DOUBLE ? 2u : 1u;
    if (format != JJS_FORMAT_AFFINE) { R = wire_pts(0); Rp = wire_pts(1); }
    verify_params P = keyset_params(scheme, c, (const uint8_t*)d[1], R, Rp, (const uint8_t*)d[4], n,
                                    out_ptrs{(uint8_t*)status, (unsigned long long*)tally, nullptr, sl->workspace});
    const uint32_t sig_stride = scheme == JJS_SCHEME_DOUBLE ? 96u : 64u;
    if (format == JJS_FORMAT_WIRE) { P.u = fe_src{(const uint8_t*)d[1], sig_stride, 0}; P.decoded_points = 1; }
    P.prep = sl->prep;
    P.pending_count = reinterpret_cast<unsigned long long*>(sl->pending.get());
    P.pending = sl->pending + 2;

    if (int rc = begin_shared(s)) return rc;
    clear_params Z{};
    Z.p[0] = tally; Z.bytes[0] = tally ? 4 * sizeof(unsigned long long) : 0;
    Z.p[1] = wire_bad(); Z.bytes[1] = n;
    Z.p[2] = sl->pending; Z.bytes[2] = sizeof(uint64_t);
    const uint64_t units = n / 16 / BLOCK + 1;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)(units < 256 ? units : 256)), dim3(BLOCK), 0, s, Z);
    if (format == JJS_FORMAT_EXT) {
        normalize_params N{};
        N.n_src = n_r;
        N.src[0] = fe_src{(const uint8_t*)d[2], 96, 0}; N.out[0] = wire_pts(0);
        N.src[1] = fe_src{(const uint8_t*)d[3], 96, 0}; N.out[1] = wire_pts(1);
        N.bad = wire_bad(); N.scratch = wire_scratch(0);
        if (int rc = launch_normalize(N, 0, n, n, s)) return rc;
    } else if (format == JJS_FORMAT_WIRE) {
        decode_params D{};
        D.n_src = n_r; D.n = n; D.first = 0; D.bad = wire_bad();
        for (uint32_t i = 0; i < n_r; ++i) { D.src[i] = fe_src{(const uint8_t*)d[1], sig_stride, 32 + 32 * i}; D.out[i] = wire_pts((int)i); }
        D.dlog = dlog_tables{g->dlog_pow, g->dlog_hash};
        if (small) {       // one lane per point: the call waits for one square root (job_hash)
            D.split = 1;
            hipLaunchKernelGGL(decode_points_kernel, dim3((unsigned)grid_for(8192, n * n_r)), dim3(BLOCK), 0, s, D);
        } else {
            hipLaunchKernelGGL(decode_kernel, dim3((unsigned)grid_for(8192, n)), dim3(BLOCK), 0, s, D);
        }
    }
    if (B)
        if (int rc = keyset_probe_launch(k, c, format, *B, n, sl->found, s)) return rc;
    keyset_front_launch(F, !small, s);
    if (small) {
        ++k.small_calls;
        const uint32_t hash_blocks = (uint32_t)((n * SB_HASH_LANES + BLOCK - 1) / BLOCK);
        const uint32_t point_blocks = (uint32_t)((n * P.resolve_lanes_keyed + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL(keyset_hash_kernel, dim3(hash_blocks + point_blocks), dim3(BLOCK), 0, s, P, hash_blocks, sl->small);
        const uint32_t positions = ks_small_positions(n);
        hipLaunchKernelGGL(keyset_small_b_kernel, dim3((unsigned)((n * positions * P.n_eq + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, P, K,
                           positions, (const uint8_t*)sl->small);
        return finish();                       // nothing is left to the resolve pass
    } else {
        ++k.large_calls;
        hipLaunchKernelGGL(prepare_kernel, dim3(grid_for(g->grid_prepare, n)), dim3(BLOCK), 0, s, P, (int)PREP_ALL, (uint64_t)0, (uint64_t)n);
        hipLaunchKernelGGL(key_verify_kernel, dim3(grid_for(g->grid_key_verify, n)), dim3(BLOCK), 0, s, P, K);
    }
    hipLaunchKernelGGL(resolve_kernel, dim3(grid_for(g->grid_resolve, n * P.resolve_lanes_keyed)), dim3(BLOCK), 0, s, P);
    return finish();
}

// bytes per item of the signature columns s0, s1, s2 of a call (0: the column is not used)
static void keyset_sig_widths(int scheme, int format, size_t w[3]) {
    const bool dbl = scheme == JJS_SCHEME_DOUBLE;
    if (format == JJS_FORMAT_WIRE) { w[0] = dbl ? 96 : 64; w[1] = 0; w[2] = 0; return; }
    w[0] = 32;
    w[1] = format == JJS_FORMAT_EXT ? 96 : 64;
    w[2] = dbl ? w[1] : 0;
}
static int keyset_check_cols(int scheme, int format, const void* key_idx, const void* s0, const void* s1, const void* s2, const void* m,
                             bool device, bool by_key = false) {
    if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
    size_t w[3];
    keyset_sig_widths(scheme, format, w);
    const void* cols[3] = {s0, s1, s2};
    // (a by-key call has no index column: its key columns are keyset_check_key_cols')
    if ((!by_key && !key_idx) || !m || (device && ((!by_key && (reinterpret_cast<uintptr_t>(key_idx) & 3u)) || !aligned16(m))))
        return fail(JJS_ERR_ARG, "null or misaligned key index or message column");
    for (int i = 0; i < 3; ++i)
        if (w[i] && (!cols[i] || (device && !aligned16(cols[i])))) return fail(JJS_ERR_ARG, "null or misaligned signature column %d", i);
    return JJS_OK;
}

// ---- blocking host calls on a device's key-set stream ------------------------------------------------------------------------
// Such a call (jjs_keyset_create, jjs_keyset_verify, the verdict algorithm of jjs_verify_all_* and jjs_keyset_verify_all)
// counts itself among g_blocking_calls in its first section under L.mu, so that jjs_shutdown does not free its device
// before it has left, and leaves through blocking_call_leave (engine_state.h) on every way out.
extern "C++" {
// The call's columns and outputs in dev's staging area (under dev->host_mu): column i of widths[i] bytes per item (0: not
// used) copied from src[i] on the key-set stream s, then up to five output areas of out_bytes[j] bytes, each part padded to 256 bytes.
struct keyset_stage {
    const void* d[6];
    uint8_t* out[5];
    hipStream_t s;
};
static int keyset_stage_in(device_state* dev, const size_t* widths, const void* const* src, size_t cols, size_t n, const size_t* out_bytes,
                           size_t outs, keyset_stage& S) {
    size_t off[11], total = 0;
    for (size_t i = 0; i < cols; ++i) { off[i] = total; total += pad256(widths[i] * n); }
    for (size_t j = 0; j < outs; ++j) { off[cols + j] = total; total += pad256(out_bytes[j]); }
    if (int rc = dev->ks_stage.ensure(total)) return rc;
    HIP_TRY(hipSetDevice(dev->device));
    S.s = dev->ks_stream;
    for (size_t i = 0; i < cols; ++i) {
        if (!widths[i]) continue;
        S.d[i] = dev->ks_stage + off[i];
        HIP_TRY(hipMemcpyAsync(dev->ks_stage + off[i], src[i], widths[i] * n, hipMemcpyHostToDevice, S.s));
    }
    for (size_t j = 0; j < outs; ++j) S.out[j] = dev->ks_stage + off[cols + j];
    return JJS_OK;
}
// The call's second section under L.mu (it holds dev->host_mu and has set g = dev): the engine still drives the same
// devices and, for a call against a set (ks non-null), the set and its copy on dev are still there; then launch(k, c).
template <class Launch>
static int keyset_launch_locked(device_state* dev, const jjs_keyset* ks, Launch launch) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
    keyset_entry* k = nullptr;
    const keyset_copy* c = nullptr;
    if (ks) {
        k = g_keysets.find(*ks);
        if (!k) return fail(JJS_ERR_ARG, "the key set was destroyed during the call");
        c = copy_for(*k, dev);
        if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    }
    return launch(k, c);
}
}  // extern "C++"

extern "C" {

int jjs_keyset_create(int scheme, int format, const uint8_t* keys, const uint8_t* keys2, size_t n_keys, uint8_t* key_status,
                      jjs_keyset* out) {
    registration<keyset_entry> call;
    if (int rc = call.enter([&] {
            if (scheme < 0 || scheme > 2 || format < 0 || format > 2) return fail(JJS_ERR_ARG, "scheme / format out of range");
            if (!out || !keys || n_keys == 0 || n_keys > KEYSET_MAX_KEYS) return fail(JJS_ERR_ARG, "a key set needs 1 .. 2^24 keys and an output handle");
            if (keyset_cols(scheme) > 1 && format != JJS_FORMAT_WIRE && !keys2) return fail(JJS_ERR_ARG, "the second key column is missing");
            return (int)JJS_OK;
        }))
        return rc;
    keyset_entry& k = *call.e;
    const uint32_t cols = keyset_cols(scheme);
    k.scheme = scheme; k.n_keys = (uint32_t)n_keys; k.n_cols = cols; k.capacity = (uint32_t)n_keys;
    k.lookup_seed = next_seed();
#if defined(JJS_PROFILING)
    if (g_pin_hash_seed) k.lookup_seed = 0;
#endif
    std::vector<uint8_t> flags;            // of the first copy: every device computes the same
    if (int rc = call.build([&](keyset_copy& c, hipStream_t s) {
            std::vector<uint8_t> f;
            const int brc = keyset_build_copy(k, c, format, keys, keys2, f, s);
            if (!brc && flags.empty()) flags.swap(f);
            return brc;
        }))
        return rc;
    uint32_t valid = 0;
    for (size_t i = 0; i < n_keys; ++i) {
        const uint32_t st = ks_key_status(flags[i], cols > 1 ? flags[n_keys + i] : (uint32_t)KT_KEY_VALID);
        if (key_status) key_status[i] = (uint8_t)st;
        valid += st == ST_OK;
    }
    k.valid = valid;
    return call.publish(g_keysets, "key set", out);
}

int jjs_keyset_destroy(jjs_keyset ks) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!g_keysets.destroy(ks)) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    return JJS_OK;
}

int jjs_keyset_info(jjs_keyset ks, uint64_t out[JJS_KEYSET_INFO]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    out[JJS_KEYSET_SCHEME] = (uint64_t)k->scheme;
    out[JJS_KEYSET_KEYS] = k->n_keys;
    out[JJS_KEYSET_VALID_KEYS] = k->valid;
    out[JJS_KEYSET_WINDOW_BITS] = (uint64_t)KEYSET_WINDOW;
    out[JJS_KEYSET_DEVICE_BYTES] = k->copies.empty() ? 0 : k->copies[0].mem.bytes();
    out[JJS_KEYSET_SMALL_CALLS] = k->small_calls;
    out[JJS_KEYSET_LARGE_CALLS] = k->large_calls;
    return JJS_OK;
}

int jjs_keyset_verify_dev(jjs_keyset ks, int format, const void* key_idx, const void* s0, const void* s1, const void* s2, const void* m,
                          size_t n, void* status, void* tally, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    hipStream_t s = (hipStream_t)stream;
    if (status && !aligned16(status)) return fail(JJS_ERR_ARG, "status must be 16-byte aligned");
    if (n == 0) {
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (tally) HIP_TRY(hipMemsetAsync(tally, 0, 4 * sizeof(unsigned long long), s));
        return JJS_OK;
    }
    if (int rc = keyset_check_cols(k->scheme, format, key_idx, s0, s1, s2, m, true)) return rc;
    const keyset_copy* c = copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    const void* d[] = {key_idx, s0, s1, s2, m};
    return no_throw([&] { return keyset_launch(*k, *c, format, d, n, status, tally, s); });
}

// A host-buffer call: the inputs go to the device's keyset staging area (4 bytes of index per item, no key), the call runs on
// the device's keyset stream, the statuses come back.  One such call at a time per device (host_mu, which jjs_trim and
// jjs_shutdown also take); the engine's mutex is held only to look the set up and to queue the launches, never while the
// call waits for the device.
int jjs_keyset_verify(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2,
                      const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]) {
    device_state* dev = nullptr;
    int scheme = 0;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (n == 0) {
            if (tally) for (int i = 0; i < 4; ++i) tally[i] = 0;
            return JJS_OK;
        }
        if (int rc = keyset_check_cols(k->scheme, format, key_idx, s0, s1, s2, m, false)) return rc;
        scheme = k->scheme;
        dev = g;
        ++g_blocking_calls;              // jjs_shutdown does not free `dev` before this call has left (see below)
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        size_t w[3];
        keyset_sig_widths(scheme, format, w);
        const size_t widths[5] = {4, w[0], w[1], w[2], 32}, out_bytes[2] = {n, 256};      // outputs: statuses, tally
        const void* src[5] = {key_idx, s0, s1, s2, m};
        keyset_stage S{};
        if (int rc = keyset_stage_in(dev, widths, src, 5, n, out_bytes, 2, S)) return rc;
        if (int rc = keyset_launch_locked(dev, &ks, [&](keyset_entry* k, const keyset_copy* c) {
                return keyset_launch(*k, *c, format, S.d, n, S.out[0], S.out[1], S.s);
            }))
            return rc;
        if (status) HIP_TRY(hipMemcpyAsync(status, S.out[0], n, hipMemcpyDeviceToHost, S.s));
        unsigned long long t[4] = {};
        HIP_TRY(hipMemcpyAsync(t, S.out[1], sizeof(t), hipMemcpyDeviceToHost, S.s));
        HIP_TRY(hipStreamSynchronize(S.s));
        if (tally) for (int i = 0; i < 4; ++i) tally[i] = t[i];
        return JJS_OK;
    });
}

// ---- by key (keyset_lookup.h): the key columns of the inline calls in place of the indices --------------------------------

int jjs_keyset_find_dev(jjs_keyset ks, int format, const void* K0, const void* K1, size_t n, void* idx_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (n == 0) return format < 0 || format > 2 ? fail(JJS_ERR_ARG, "format out of range") : (int)JJS_OK;
    if (int rc = keyset_check_key_cols(k->n_cols, format, K0, K1, true)) return rc;
    if (!idx_out || (reinterpret_cast<uintptr_t>(idx_out) & 3u)) return fail(JJS_ERR_ARG, "null or misaligned index output");
    const keyset_copy* c = copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    const keyset_by_key B{K0, K1, idx_out};
    return no_throw([&] { return keyset_find_launch(*k, *c, format, B, n, (hipStream_t)stream); });
}

// From host buffers, blocking: the route of jjs_keyset_verify (the device's keyset staging area and stream, under host_mu).
int jjs_keyset_find(jjs_keyset ks, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint32_t* idx_out) {
    device_state* dev = nullptr;
    uint32_t cols = 0;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (n == 0) return JJS_OK;
        if (int rc = keyset_check_key_cols(k->n_cols, format, K0, K1, false)) return rc;
        if (!idx_out) return fail(JJS_ERR_ARG, "null index output");
        cols = k->n_cols;
        dev = g;
        ++g_blocking_calls;
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        size_t kw[2];
        keyset_key_widths(cols, format, kw);
        const size_t out_bytes[1] = {n * 4};
        const void* src[2] = {K0, K1};
        keyset_stage S{};
        if (int rc = keyset_stage_in(dev, kw, src, 2, n, out_bytes, 1, S)) return rc;
        if (int rc = keyset_launch_locked(dev, &ks, [&](keyset_entry* k, const keyset_copy* c) {
                return keyset_find_launch(*k, *c, format, keyset_by_key{S.d[0], S.d[1], S.out[0]}, n, S.s);
            }))
            return rc;
        HIP_TRY(hipMemcpyAsync(idx_out, S.out[0], n * 4, hipMemcpyDeviceToHost, S.s));
        HIP_TRY(hipStreamSynchronize(S.s));
        return JJS_OK;
    });
}

int jjs_keyset_verify_keys_dev(jjs_keyset ks, int format, const void* K0, const void* K1, const void* s0, const void* s1, const void* s2,
                               const void* m, size_t n, void* status, void* tally, void* idx_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    hipStream_t s = (hipStream_t)stream;
    if (status && !aligned16(status)) return fail(JJS_ERR_ARG, "status must be 16-byte aligned");
    if (n == 0) {
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (tally) HIP_TRY(hipMemsetAsync(tally, 0, 4 * sizeof(unsigned long long), s));
        return JJS_OK;
    }
    if (int rc = keyset_check_cols(k->scheme, format, nullptr, s0, s1, s2, m, true, true)) return rc;
    if (int rc = keyset_check_key_cols(k->n_cols, format, K0, K1, true)) return rc;
    if (reinterpret_cast<uintptr_t>(idx_out) & 3u) return fail(JJS_ERR_ARG, "misaligned index output");
    const keyset_copy* c = copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    const void* d[] = {nullptr, s0, s1, s2, m};
    const keyset_by_key B{K0, K1, idx_out};
    return no_throw([&] { return keyset_launch(*k, *c, format, d, n, status, tally, s, &B); });
}

}  // extern "C"

// The inline host entry point of a scheme and format over the columns of a by-key call: col = K0, K1, s0, s1, s2, m.
static int keyset_inline_host(int scheme, int format, const uint8_t* const* col, size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t *K0 = col[0], *K1 = col[1], *s0 = col[2], *s1 = col[3], *s2 = col[4], *m = col[5];
    if (format == JJS_FORMAT_WIRE)
        return scheme == JJS_SCHEME_SINGLE ? jjs_verify_single_wire(s0, K0, m, n, status, tally)
             : scheme == JJS_SCHEME_DOUBLE ? jjs_verify_double_wire(s0, K0, m, n, status, tally)
                                           : jjs_verify_vargen_wire(s0, K0, m, n, status, tally);
    if (format == JJS_FORMAT_EXT)
        return scheme == JJS_SCHEME_SINGLE ? jjs_verify_single_ext(s0, s1, K0, m, n, status, tally)
             : scheme == JJS_SCHEME_DOUBLE ? jjs_verify_double_ext(s0, s1, s2, K0, K1, m, n, status, tally)
                                           : jjs_verify_vargen_ext(s0, s1, K0, K1, m, n, status, tally);
    return scheme == JJS_SCHEME_SINGLE ? jjs_verify_single(s0, s1, K0, m, n, status, tally)
         : scheme == JJS_SCHEME_DOUBLE ? jjs_verify_double(s0, s1, s2, K0, K1, m, n, status, tally)
                                       : jjs_verify_vargen(s0, s1, K0, K1, m, n, status, tally);
}
// The items of a by-key host call whose key is not in the set (status KL_STATUS_NOT_IN_SET in st): their rows gathered, verified
// by the inline host entry point, their statuses scattered back and their tally added.  Nothing runs when there is none.
static int keyset_verify_misses_inline(int scheme, uint32_t cols, int format, const uint8_t* const* col, size_t n, uint8_t* st, uint64_t t[4]) {
    std::vector<size_t> miss;
    for (size_t i = 0; i < n; ++i)
        if (st[i] == KL_STATUS_NOT_IN_SET) miss.push_back(i);
    if (miss.empty()) return JJS_OK;
    size_t w[6];
    keyset_key_widths(cols, format, w);
    keyset_sig_widths(scheme, format, w + 2);
    w[5] = 32;
    std::vector<uint8_t> rows[6], out(miss.size());
    const uint8_t* p[6] = {};
    for (int c = 0; c < 6; ++c) {
        if (!w[c]) continue;
        rows[c].resize(miss.size() * w[c]);
        for (size_t j = 0; j < miss.size(); ++j) memcpy(rows[c].data() + j * w[c], col[c] + miss[j] * w[c], w[c]);
        p[c] = rows[c].data();
    }
    uint64_t mt[4] = {};
    if (int rc = keyset_inline_host(scheme, format, p, miss.size(), out.data(), mt)) return rc;
    for (size_t j = 0; j < miss.size(); ++j) st[miss[j]] = out[j];
    for (int i = 0; i < 4; ++i) t[i] += mt[i];
    return JJS_OK;
}

extern "C" {

// The drop-in of jjs_verify_{single,double,vargen}{,_ext,_wire}: the by-key call on the host route of jjs_keyset_verify, then --
// only when a key was not in the set, and with host_mu released, because large inline host calls take it -- the inline call
// over the missed rows.  Statuses and tally are those of the inline call over all n items.
int jjs_keyset_verify_keys(jjs_keyset ks, int format, const uint8_t* K0, const uint8_t* K1, const uint8_t* s0, const uint8_t* s1,
                           const uint8_t* s2, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4], uint32_t* idx_out) {
    device_state* dev = nullptr;
    int scheme = 0;
    uint32_t cols = 0;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
        if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
        if (n == 0) {
            if (tally) for (int i = 0; i < 4; ++i) tally[i] = 0;
            return JJS_OK;
        }
        if (int rc = keyset_check_cols(k->scheme, format, nullptr, s0, s1, s2, m, false, true)) return rc;
        if (int rc = keyset_check_key_cols(k->n_cols, format, K0, K1, false)) return rc;
        scheme = k->scheme; cols = k->n_cols;
        dev = g;
        ++g_blocking_calls;
    }
    std::vector<uint8_t> own;              // the statuses when the caller wants none: the misses are read from them
    uint8_t* st = status;
    uint64_t t[4] = {};
    {
        blocking_call_leave leave_on_every_way_out;
        std::lock_guard<std::mutex> big(dev->host_mu);
        g = dev;
        const int rc = no_throw([&]() -> int {
            if (!st) { own.resize(n); st = own.data(); }
            size_t w[6];
            keyset_key_widths(cols, format, w);
            keyset_sig_widths(scheme, format, w + 2);
            w[5] = 32;
            const size_t out_bytes[3] = {n, 256, n * 4};      // outputs: statuses, tally, indices
            const void* src[6] = {K0, K1, s0, s1, s2, m};
            keyset_stage S{};
            if (int rc = keyset_stage_in(dev, w, src, 6, n, out_bytes, 3, S)) return rc;
            const void* d[] = {nullptr, S.d[2], S.d[3], S.d[4], S.d[5]};
            const keyset_by_key B{S.d[0], S.d[1], S.out[2]};
            if (int rc = keyset_launch_locked(dev, &ks, [&](keyset_entry* k, const keyset_copy* c) {
                    return keyset_launch(*k, *c, format, d, n, S.out[0], S.out[1], S.s, &B);
                }))
                return rc;
            HIP_TRY(hipMemcpyAsync(st, S.out[0], n, hipMemcpyDeviceToHost, S.s));
            unsigned long long dt[4] = {};
            HIP_TRY(hipMemcpyAsync(dt, S.out[1], sizeof(dt), hipMemcpyDeviceToHost, S.s));
            if (idx_out) HIP_TRY(hipMemcpyAsync(idx_out, S.out[2], n * 4, hipMemcpyDeviceToHost, S.s));
            HIP_TRY(hipStreamSynchronize(S.s));
            for (int i = 0; i < 4; ++i) t[i] = dt[i];
            return JJS_OK;
        });
        if (rc) return rc;
    }
    const uint8_t* col[6] = {K0, K1, s0, s1, s2, m};
    if (int rc = no_throw([&] { return keyset_verify_misses_inline(scheme, cols, format, col, n, st, t); })) return rc;
    if (tally) for (int i = 0; i < 4; ++i) tally[i] = t[i];
    return JJS_OK;
}

}  // extern "C"

// Part of jjs_gpu.hip (included among the extern "C" entry points, behind keyset_add_calls.h, whose alloc and leave helpers it
// uses): removing keys from a registered key set and compacting it (include/jjs_gpu.h jjs_keyset_remove, jjs_keyset_compact,
// jjs_keyset_removal; the device side is keyset_remove.h).
//
// Like an add, one remove or compact runs at a time per set and never beside an add or a reserve (keyset_entry::growing); it
// counts among the blocking calls jjs_shutdown waits for and among those jjs_trim waits for (g_keyset_grows), runs outside the
// engine's mutex on a stream of its own per device, and publishes its counts under the mutex.
//
// UNLIKE an add, a remove writes what queued launches read: flag bytes and lookup slots of ids below their n_keys.  What such a
// launch may see:
//   flag bytes     go one way, from the key's flags to MALFORMED | REMOVED without VALID: a launch reads the byte before or after;
//   lookup slots   a slot goes from the id to KA_RETRACTED, and a higher duplicate may enter an empty slot: a probe finds the
//                  removed id, nothing, or the lowest surviving duplicate;
//   rows, tables, on-curve bytes, the words block: not written.
// A remove that fails on one device of several has removed the keys on the devices before it; the entry's counts change only on
// success, and the call may be repeated: removing is idempotent on the device (the repeated call then counts, on the devices that
// had done it, nothing -- so the answers and the counts are taken from the LAST device, which has done it once).
//
// A compact moves the set as a moving add does: a new allocation in the layout jjs_keyset_create gives a set of the survivors,
// the old one retired under the mutex.  Queued launches go on reading the old allocation with the old indices.

extern "C++" {
// The regions of an allocation that holds exactly n keys, in jjs_keyset_create's layout (null base: only the size is wanted).
static size_t keyset_carve_created(keyset_regions& r, uint8_t* base, uint32_t cols, uint32_t n) {
    const size_t key_bytes = pad256((size_t)n * 64), flag_bytes = pad256(n), table_bytes = pad256((size_t)n * keyset_table_bytes_per_key());
    const uint32_t slots = kl_slot_count(n);
    uint8_t* p = base;
    r = keyset_regions{};
    r.words = reinterpret_cast<uint32_t*>(p); p += 256;
    for (uint32_t i = 0; i < cols; ++i) {
        r.keys[i] = p; p += key_bytes;
        r.flags[i] = p; p += flag_bytes;
        r.tables[i] = reinterpret_cast<uint32_t*>(p); p += table_bytes;
    }
    r.lookup = reinterpret_cast<uint32_t*>(p); p += pad256((size_t)slots * 4);
    r.lookup_mask = slots - 1;
    r.on_curve = p; p += flag_bytes;
    return (size_t)(p - base);
}

struct keyset_shrink_job {
    device_state* dev = nullptr;
    keyset_regions old, now;
    device_mem<uint8_t> fresh, tmp;
    stream_owner s;
};
// What both calls read of the set under L.mu on the way in.
struct keyset_shrink_call {
    uint32_t cols = 0, n_keys = 0, removed = 0;
    uint64_t seed = 0;
};
static keyset_lookup keyset_shrink_lookup(const keyset_shrink_call& A, const keyset_regions& r, uint32_t n_keys) {
    keyset_lookup T{};
    for (uint32_t i = 0; i < A.cols; ++i) { T.keys[i] = r.keys[i]; T.flags[i] = r.flags[i]; }
    T.on_curve = r.on_curve; T.slots = r.lookup; T.mask = r.lookup_mask;
    T.n_keys = n_keys; T.n_cols = A.cols; T.seed = A.seed;
    return T;
}

// The first section of a remove or a compact under L.mu: the set found and free (waiting for an add, reserve, remove or compact
// at work), check(k) passed, then the jobs filled and the call counted in.  `done` is set when check() answered the call.
template <class Check>
static int keyset_shrink_enter(jjs_keyset ks, keyset_shrink_call& A, std::vector<device_state*>& devs,
                               std::vector<std::unique_ptr<keyset_shrink_job>>& jobs, bool* done, Check check) {
    std::unique_lock<std::mutex> lock(L.mu);
    keyset_entry* k = nullptr;
    for (;;) {
        if (int rc = check_ready()) return rc;
        k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
        if (!k->growing) break;
        L.lane_cv.wait(lock);
    }
    if (int rc = check(*k, done)) return rc;
    if (*done) return JJS_OK;
    A.cols = k->n_cols; A.n_keys = k->n_keys; A.removed = k->removed; A.seed = k->lookup_seed;
    if (int rc = no_throw([&] {
            devs = L.devs;
            for (size_t i = 0; i < k->copies.size(); ++i) jobs.emplace_back(new keyset_shrink_job());
            return k->copies.size() == devs.size() ? (int)JJS_OK : fail(JJS_ERR_NOT_INIT, "the key set was built for other devices");
        }))
        return rc;
    for (size_t i = 0; i < jobs.size(); ++i) {
        jobs[i]->dev = k->copies[i].dev;
        jobs[i]->old = static_cast<const keyset_regions&>(k->copies[i]);
    }
    k->growing = true;
    ++g_blocking_calls;
    ++g_keyset_grows;
    return JJS_OK;
}

// One device's share of a remove (g is that device): the four launches of keyset_remove.h, the answers and the counts back.
static int keyset_remove_on(const keyset_shrink_call& A, keyset_shrink_job& J, const uint32_t* idx, uint32_t n, uint8_t* result, uint32_t counts[2]) {
    const size_t idx_bytes = pad256((size_t)n * 4), res_bytes = pad256(n);
    if (int rc = keyset_grow_alloc(J.tmp, idx_bytes + res_bytes + 256, "a key set's remove area")) return rc;
    hipStream_t s = J.s;
    keyset_remove_plan P{};
    P.T = keyset_shrink_lookup(A, J.old, A.n_keys);
    P.flags[0] = J.old.flags[0]; P.flags[1] = J.old.flags[1];
    uint8_t* q = J.tmp;
    P.idx = reinterpret_cast<const uint32_t*>(q); q += idx_bytes;
    P.result = q; q += res_bytes;
    P.counts = reinterpret_cast<uint32_t*>(q);
    P.n = n;
    const unsigned blocks = (n + BLOCK - 1) / BLOCK;
    const int rc = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(J.tmp.get(), idx, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(P.counts, 0, 256, s));
        hipLaunchKernelGGL(keyset_remove_answer_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
        hipLaunchKernelGGL(keyset_remove_flags_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
        hipLaunchKernelGGL(keyset_remove_retract_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
        hipLaunchKernelGGL(keyset_remove_reenter_kernel, dim3((A.n_keys + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, P.T);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(result, P.result, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(counts, P.counts, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    }();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

// One device's share of a compact (g is that device): the new allocation filled from the old one; map_out (n_keys words, host).
static int keyset_compact_on(const keyset_shrink_call& A, keyset_shrink_job& J, uint32_t n_new, uint32_t* map_out) {
    const uint32_t cols = A.cols, n = A.n_keys, blocks = (n + BLOCK - 1) / BLOCK;
    const size_t bytes = keyset_carve_created(J.now, nullptr, cols, n_new);
    if (int rc = keyset_grow_alloc(J.fresh, bytes, "a compacted key set")) return rc;
    keyset_carve_created(J.now, J.fresh, cols, n_new);
    const size_t sums_bytes = pad256(((size_t)blocks + 1) * 4), src_bytes = pad256((size_t)n_new * 4), map_bytes = pad256((size_t)n * 4);
    if (int rc = keyset_grow_alloc(J.tmp, sums_bytes + src_bytes + map_bytes, "a key set's compact area")) return rc;
    hipStream_t s = J.s;
    keyset_compact_plan P{};
    for (uint32_t i = 0; i < cols; ++i) {
        P.keys[i] = J.old.keys[i]; P.flags[i] = J.old.flags[i];
        P.new_keys[i] = J.now.keys[i]; P.new_flags[i] = J.now.flags[i];
    }
    P.on_curve = J.old.on_curve; P.new_on_curve = J.now.on_curve;
    uint8_t* q = J.tmp;
    P.sums = reinterpret_cast<uint32_t*>(q); q += sums_bytes;
    P.src = reinterpret_cast<uint32_t*>(q); q += src_bytes;
    P.map = reinterpret_cast<uint32_t*>(q);
    P.n_keys = n; P.n_cols = cols;
    keyset_table_gather G{};
    for (uint32_t i = 0; i < cols; ++i) { G.old_tables[i] = J.old.tables[i]; G.new_tables[i] = J.now.tables[i]; }
    G.src = P.src; G.n_new = n_new; G.n_cols = cols;
    G.units = (uint32_t)(keyset_table_bytes_per_key() / 16);
    G.slices = (G.units + KR_TABLE_SLICE - 1) / KR_TABLE_SLICE;
    const uint64_t pieces = (uint64_t)G.slices * n_new * cols;
    const uint32_t words[64] = {n_new, n_new, (uint32_t)KEYSET_WINDOW};       // (host memory the queued copy reads: the stream is drained below)
    uint32_t total = 0;
    const int rc = [&]() -> int {
        if (keyset_table_bytes_per_key() % 16) return fail(JJS_ERR_HIP, "a key's tables are no multiple of 16 bytes");
        HIP_TRY(hipMemcpyAsync(J.now.words, words, sizeof(words), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(keyset_compact_mark_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
        hipLaunchKernelGGL(keyset_add_scan_kernel, dim3(1), dim3(KA_SCAN_LANES), 0, s, P.sums, blocks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&total, P.sums + blocks, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // (the gather writes n_new rows: not before the device's own count agrees with the entry's)
        if (total != n_new) return fail(JJS_ERR_HIP, "the device counts %u surviving keys, the engine %u", total, n_new);
        hipLaunchKernelGGL(keyset_compact_gather_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
        hipLaunchKernelGGL(keyset_table_gather_kernel, dim3((unsigned)(pieces < (1u << 20) ? pieces : (1u << 20))), dim3(BLOCK), 0, s, G, pieces);
        keyset_lookup T = keyset_shrink_lookup(A, J.now, n_new);
        HIP_TRY(hipMemsetAsync(T.slots, 0xFF, ((size_t)T.mask + 1) * 4, s));
        hipLaunchKernelGGL(keyset_lookup_insert_kernel, dim3((n_new + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, T);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(map_out, P.map, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    }();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}
}  // extern "C++"

extern "C" {

int jjs_keyset_remove(jjs_keyset ks, const uint32_t* idx, size_t n, uint8_t* result, size_t* n_removed) {
    keyset_shrink_call A;
    std::vector<device_state*> devs;
    std::vector<std::unique_ptr<keyset_shrink_job>> jobs;
    bool done = false;
    if (int rc = keyset_shrink_enter(ks, A, devs, jobs, &done, [&](keyset_entry& k, bool* answered) -> int {
            if (n == 0) {
                if (n_removed) *n_removed = 0;
                *answered = true;
                return JJS_OK;
            }
            if (!idx) return fail(JJS_ERR_ARG, "null index column");
            if (n > 0xFFFFFFFFu) return fail(JJS_ERR_ARG, "too many indices");
            k.removed_from = true;
            return JJS_OK;
        }))
        return rc;
    if (done) return JJS_OK;
    keyset_grow_leave leave_on_every_way_out{ks};
    std::vector<uint8_t> res;
    uint32_t counts[2] = {};
    if (int rc = no_throw([&]() -> int {
            device_restore restore;
            res.resize(n);
            for (auto& job : jobs) {
                keyset_shrink_job& J = *job;
                g = J.dev;
                HIP_TRY(hipSetDevice(J.dev->device));
                HIP_TRY(J.s.create(hipStreamNonBlocking));
                if (int e = keyset_remove_on(A, J, idx, (uint32_t)n, res.data(), counts)) return e;     // (every device answers the same; see above)
                J.tmp = device_mem<uint8_t>();          // (its stream is drained)
            }
            return JJS_OK;
        }))
        return rc;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "the key set was destroyed during the call");
        k->removed += counts[0];
        k->valid -= counts[1];
        ++k->remove_calls;
    }
    if (result) memcpy(result, res.data(), n);
    if (n_removed) *n_removed = counts[0];
    return JJS_OK;
}

int jjs_keyset_compact(jjs_keyset ks, uint32_t* map_out, size_t map_len, size_t* n_keys_out) {
    keyset_shrink_call A;
    std::vector<device_state*> devs;
    std::vector<std::unique_ptr<keyset_shrink_job>> jobs;
    bool done = false;
    if (int rc = keyset_shrink_enter(ks, A, devs, jobs, &done, [&](keyset_entry& k, bool* answered) -> int {
            if (map_out && map_len != k.n_keys) return fail(JJS_ERR_ARG, "the map must hold one word per key of the set");
            if (k.removed == k.n_keys) return fail(JJS_ERR_ARG, "every key of the set is removed: destroy it");
            if (k.removed == 0) {
                if (map_out) for (uint32_t i = 0; i < k.n_keys; ++i) map_out[i] = i;
                if (n_keys_out) *n_keys_out = k.n_keys;
                *answered = true;
            }
            return JJS_OK;
        }))
        return rc;
    if (done) return JJS_OK;
    keyset_grow_leave leave_on_every_way_out{ks};
    const uint32_t n_new = A.n_keys - A.removed;
    std::vector<uint32_t> map;
    if (int rc = no_throw([&]() -> int {
            device_restore restore;
            map.resize(A.n_keys);
            for (auto& job : jobs) {
                keyset_shrink_job& J = *job;
                g = J.dev;
                HIP_TRY(hipSetDevice(J.dev->device));
                HIP_TRY(J.s.create(hipStreamNonBlocking));
                if (int e = keyset_compact_on(A, J, n_new, map.data())) return e;       // (every device computes the same map)
                J.tmp = device_mem<uint8_t>();
            }
            return JJS_OK;
        }))
        return rc;               // (nothing was published; the new allocations are freed with `jobs`: every stream is drained)
    {
        std::lock_guard<std::mutex> lock(L.mu);
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "the key set was destroyed during the call");
        if (L.devs != devs || k->copies.size() != jobs.size()) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
        device_state* const keep = g;
        for (size_t i = 0; i < jobs.size(); ++i) {      // launches already queued still read the old allocation: retired, as a destroyed set's
            keyset_copy& c = k->copies[i];
            static_cast<keyset_regions&>(c) = jobs[i]->now;
            g = c.dev;
            c.mem.replace(std::move(jobs[i]->fresh));
            for (auto& m : c.side) m.release();
            c.side.clear();
            c.word_blocks = 0;
        }
        g = keep;
        k->n_keys = n_new; k->capacity = n_new; k->removed = 0;
        ++k->compact_calls;
        ++k->growth[JJS_KEYSET_RELOCATIONS];
    }
    if (map_out) memcpy(map_out, map.data(), (size_t)A.n_keys * 4);
    if (n_keys_out) *n_keys_out = n_new;
    return JJS_OK;
}

int jjs_keyset_removal(jjs_keyset ks, uint64_t out[JJS_KEYSET_REMOVAL]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    out[JJS_KEYSET_REMOVED_KEYS] = k->removed;
    out[JJS_KEYSET_LIVE_KEYS] = k->n_keys - k->removed;
    out[JJS_KEYSET_REMOVE_CALLS] = k->remove_calls;
    out[JJS_KEYSET_COMPACT_CALLS] = k->compact_calls;
    return JJS_OK;
}

}  // extern "C"

// Part of jjs_gpu.hip (included among the extern "C" entry points, behind keyset_calls.h): growing a registered key set
// (include/jjs_gpu.h jjs_keyset_add, jjs_keyset_reserve, jjs_keyset_growth; the device side is keyset_add.h).
//
// One add or reserve runs at a time per set (keyset_entry::growing; the next waits on the engine's condition variable).  Like
// jjs_keyset_create it counts among the blocking calls jjs_shutdown waits for, builds outside the engine's mutex on a stream of
// its own per device, and publishes n_keys, valid, the capacity and the pointers of every copy under the mutex once every
// driven device's copy is complete.  Until then nothing a launch of the old set can read has changed:
//   rows, flags, tables                   are written beyond n_old only;
//   on-curve bytes                        likewise -- except that a rebuild of the lookup table enters every id anew, and kl_insert
//                                         stores the on-curve byte of each: the old ids' bytes are written again WITH THE VALUES
//                                         THEY HOLD (a function of rows and flags that did not change), which a reader cannot tell
//                                         from no write;
//   the lookup table                      gets the new ids in place (keyset_add.h: why probes of the old set do not see them),
//                                         or is built anew, with more slots, in a region of its own -- a grown allocation holds
//                                         2 x kl_slot_count(capacity) slots, and the table of s slots lies at slot offset s, so
//                                         the tables of all the slot counts the capacity allows lie side by side;
//   the words block                       (n_keys, n_keys, window: key_params::counters and verify_params::key_flag of queued
//                                         launches point at it) is never overwritten: every published size gets a block of its
//                                         own, the first of an allocation inside it, the later ones in small allocations beside
//                                         it (keyset_copy::side), which retire with it.
// A set that does not fit its capacity moves: a larger allocation, device-to-device copies of what the old keys own, the new
// keys built behind them, and the old allocation retired under the mutex as jjs_keyset_destroy retires it.
// jjs_trim frees retired memory; it waits for adds in progress (g_keyset_grows), because a set that is destroyed while it grows
// in place is retired memory the add still writes.  Such an add finds its handle stale when it comes to publish and returns -1.
// A failed add publishes nothing.  What it wrote beyond n_old is written again by the next add.  The lookup insert is its last
// launch, but an add can still fail behind it (another device's build, the devices changed, no memory for the publication), and
// an add in place has then entered ids >= n_keys into the live table.  While they are >= n_keys every probe skips them; but a
// later add registers OTHER keys at those indices, and a key could then be met at such a slot ahead of its own, hiding a lower
// index of an equal key.  So a failing add retracts them (keyset_grow_retract, ka_retract in keyset_add.h): the slots stay taken
// and never hit.  They count against the half-full bound -- up to n_added slots per failed add in place -- until the next
// rebuild starts from an empty table.  (A set destroyed under the add needs none of this: nothing reads it again.)

constexpr uint32_t KEYSET_WORD_BLOCKS = 16;       // 256-byte words blocks per side allocation

extern "C++" {
static size_t keyset_table_bytes_per_key() { return (size_t)kt_positions(KEYSET_WINDOW) * kt_table_words(KEYSET_WINDOW) * 4; }
// The regions of an allocation that holds room for `cap` keys, carved from `base` (null: only the size is wanted).
static size_t keyset_carve_grown(keyset_regions& r, uint8_t* base, uint32_t cols, uint32_t cap) {
    const size_t key_bytes = pad256((size_t)cap * 64), flag_bytes = pad256(cap), table_bytes = pad256((size_t)cap * keyset_table_bytes_per_key());
    const uint32_t room = 2 * kl_slot_count(cap);
    uint8_t* p = base;
    r = keyset_regions{};
    r.words = reinterpret_cast<uint32_t*>(p); p += 256;
    for (uint32_t i = 0; i < cols; ++i) {
        r.keys[i] = p; p += key_bytes;
        r.flags[i] = p; p += flag_bytes;
        r.tables[i] = reinterpret_cast<uint32_t*>(p); p += table_bytes;
    }
    r.lookup = reinterpret_cast<uint32_t*>(p); p += pad256((size_t)room * 4);       // (the region: the caller places the table in it)
    r.on_curve = p; p += flag_bytes;
    r.lookup_room = room;
    return (size_t)(p - base);
}

// One device's share of a growth call.
struct keyset_grow_job {
    device_state* dev = nullptr;
    keyset_regions old, now;               // as published when the call came in / as it will publish them
    uint8_t* side_back = nullptr;          // the copy's last side allocation and its blocks taken, when the call came in
    uint32_t word_blocks = 0;
    device_mem<uint8_t> fresh;             // a move: the new allocation
    device_mem<uint8_t> fresh_side;        // in place: a new side allocation, when the last one is full
    bool took_block = false;               // in place: a words block was taken
    bool entered_in_place = false;         // in place: new ids were entered into the LIVE lookup table
    stream_owner s;
    device_mem<uint8_t> tmp_a, tmp_b;      // build areas: the candidates and the plan / the chains of the new keys
    keyset_add_plan P{};
    uint8_t* cand[2] = {};
    uint8_t* bad = nullptr;
    uint32_t* idx_dev = nullptr;
    uint8_t* status_dev = nullptr;
};
// What a growth call knows of the set (read under L.mu) and decides on the way.
struct keyset_grow_call {
    int scheme = 0, format = 0, mode = 0;
    uint32_t cols = 0, n_old = 0, cap = 0, n = 0;
    uint64_t seed = 0;
    uint32_t n_add = 0, n_new = 0, new_cap = 0;     // new_cap != cap: the copies move
    bool rebuild = false;                           // the lookup table gets more slots
    const uint8_t* src[2] = {};
};

static int keyset_grow_alloc(device_mem<uint8_t>& m, size_t bytes, const char* what) {
    if (m.alloc(bytes ? bytes : 256) != hipSuccess) {
        (void)hipGetLastError();
        return fail(JJS_ERR_HIP, "hipMalloc of %s (%zu bytes) failed", what, bytes);
    }
    return JJS_OK;
}

// Stage A on one device (g is that device): the candidates uploaded and decoded / normalised / copied into rows of the build
// area, and for JJS_KEYSET_ADD_UNIQUE the probe, the claim and the scan; *n_first receives the number of first occurrences
// (APPEND: n).  The stream is drained on the way out.
static int keyset_grow_plan(const keyset_grow_call& A, keyset_grow_job& J, uint32_t* n_first) {
    const uint32_t n = A.n, cols = A.cols;
    const bool unique = A.mode == JJS_KEYSET_ADD_UNIQUE;
    const size_t in_width = A.format == JJS_FORMAT_EXT ? 96 : (A.format == JJS_FORMAT_WIRE ? 32 : 0);
    const size_t in_bytes = pad256((size_t)n * in_width * cols), row_bytes = pad256((size_t)n * 64), byte_bytes = pad256(n), word_bytes = pad256((size_t)n * 4);
    const uint32_t blocks = (n + BLOCK - 1) / BLOCK, cslots = kl_slot_count(n);
    size_t total = in_bytes + cols * row_bytes + byte_bytes + pad256((size_t)n * 48) + word_bytes + byte_bytes;
    if (unique) total += 3 * byte_bytes + 3 * word_bytes + pad256(((size_t)blocks + 1) * 4) + pad256((size_t)cslots * 4);
    if (int rc = keyset_grow_alloc(J.tmp_a, total, "a key set's build area")) return rc;
    hipStream_t s = J.s;
    uint8_t* q = J.tmp_a;
    uint8_t* in = q; q += in_bytes;
    for (uint32_t i = 0; i < cols; ++i) { J.cand[i] = q; q += row_bytes; }
    J.bad = q; q += byte_bytes;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(q); q += pad256((size_t)n * 48);
    J.idx_dev = reinterpret_cast<uint32_t*>(q); q += word_bytes;
    J.status_dev = q; q += byte_bytes;
    const int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(J.bad, 0, byte_bytes, s));
        if (A.format == JJS_FORMAT_AFFINE) {
            for (uint32_t i = 0; i < cols; ++i) HIP_TRY(hipMemcpyAsync(J.cand[i], A.src[i], (size_t)n * 64, hipMemcpyHostToDevice, s));
        } else if (A.format == JJS_FORMAT_EXT) {
            normalize_params N{};
            for (uint32_t i = 0; i < cols; ++i) {
                HIP_TRY(hipMemcpyAsync(in + (size_t)i * n * 96, A.src[i], (size_t)n * 96, hipMemcpyHostToDevice, s));
                N.src[i] = fe_src{in + (size_t)i * n * 96, 96, 0};
                N.out[i] = J.cand[i];
            }
            N.n_src = cols; N.bad = J.bad; N.scratch = scratch;
            if (int e = launch_normalize(N, 0, n, n, s)) return e;
        } else {
            HIP_TRY(hipMemcpyAsync(in, A.src[0], (size_t)n * 32 * cols, hipMemcpyHostToDevice, s));
            decode_params D{};
            D.n_src = cols; D.n = n; D.bad = J.bad;
            for (uint32_t i = 0; i < cols; ++i) { D.src[i] = fe_src{in, 32 * cols, 32 * i}; D.out[i] = J.cand[i]; }
            D.dlog = dlog_tables{g->dlog_pow, g->dlog_hash};
            hipLaunchKernelGGL(decode_kernel, dim3((unsigned)grid_for(8192, n)), dim3(BLOCK), 0, s, D);
        }
        *n_first = n;
        if (unique) {
            keyset_add_plan& P = J.P;
            P = keyset_add_plan{};
            P.skip = q; q += byte_bytes;
            P.first = q; q += byte_bytes;
            uint8_t* c_on_curve = q; q += byte_bytes;
            P.res = reinterpret_cast<uint32_t*>(q); q += word_bytes;
            P.lead = reinterpret_cast<uint32_t*>(q); q += word_bytes;
            P.rank = reinterpret_cast<uint32_t*>(q); q += word_bytes;
            P.sums = reinterpret_cast<uint32_t*>(q); q += pad256(((size_t)blocks + 1) * 4);
            uint32_t* slots = reinterpret_cast<uint32_t*>(q); q += pad256((size_t)cslots * 4);
            for (uint32_t i = 0; i < cols; ++i) {
                P.S.keys[i] = J.old.keys[i]; P.S.flags[i] = J.old.flags[i];
                P.C.keys[i] = J.cand[i]; P.C.flags[i] = P.skip;
            }
            P.S.on_curve = J.old.on_curve; P.S.slots = J.old.lookup; P.S.mask = J.old.lookup_mask;
            P.S.n_keys = A.n_old; P.S.n_cols = cols; P.S.seed = A.seed;
            P.C.on_curve = c_on_curve; P.C.slots = slots; P.C.mask = cslots - 1;
            P.C.n_keys = n; P.C.n_cols = cols; P.C.seed = A.seed;
            P.bad = J.bad; P.n = n; P.n_old = A.n_old;
            HIP_TRY(hipMemsetAsync(slots, 0xFF, (size_t)cslots * 4, s));
            hipLaunchKernelGGL(keyset_add_probe_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
            hipLaunchKernelGGL(keyset_add_claim_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
            hipLaunchKernelGGL(keyset_add_mark_kernel, dim3(blocks), dim3(BLOCK), 0, s, P);
            hipLaunchKernelGGL(keyset_add_scan_kernel, dim3(1), dim3(KA_SCAN_LANES), 0, s, P.sums, blocks);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(n_first, P.sums + blocks, 4, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    }();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

// Stage B on one device (g is that device): the move or the in-place extension, the new keys' rows, flags, chains, tables and
// lookup entries, the words block of the new size, and the answers.  flags_out (cols x n_add), idx_out and status_out (n each;
// UNIQUE only) are host memory.  The stream is drained on the way out.
static int keyset_grow_build(const keyset_grow_call& A, keyset_grow_job& J, uint8_t* flags_out, uint32_t* idx_out, uint8_t* status_out) {
    const uint32_t cols = A.cols, n_old = A.n_old, n_add = A.n_add, n_new = A.n_new;
    const int w = KEYSET_WINDOW;
    const bool unique = A.mode == JJS_KEYSET_ADD_UNIQUE, moving = A.new_cap != A.cap;
    const size_t per_key = keyset_table_bytes_per_key();
    hipStream_t s = J.s;
    // host memory the queued copies read: it outlives the stream, which is drained on every way out
    std::vector<uint32_t> ids(n_add);
    for (uint32_t i = 0; i < n_add; ++i) ids[i] = i;
    const uint32_t words[64] = {n_new, n_new, (uint32_t)w}, counters[64] = {n_add, n_add, (uint32_t)w};
    const int rc = [&]() -> int {
        const uint32_t s_old = J.old.lookup_mask + 1, s_new = kl_slot_count(n_new);
        if (moving) {
            keyset_regions r;
            const size_t bytes = keyset_carve_grown(r, nullptr, cols, A.new_cap);
            if (int e = keyset_grow_alloc(J.fresh, bytes, "a grown key set")) return e;
            keyset_carve_grown(J.now, J.fresh, cols, A.new_cap);
            uint32_t* const region = J.now.lookup;
            for (uint32_t i = 0; i < cols; ++i) {
                HIP_TRY(hipMemcpyAsync(J.now.keys[i], J.old.keys[i], (size_t)n_old * 64, hipMemcpyDeviceToDevice, s));
                HIP_TRY(hipMemcpyAsync(J.now.flags[i], J.old.flags[i], n_old, hipMemcpyDeviceToDevice, s));
                HIP_TRY(hipMemcpyAsync(J.now.tables[i], J.old.tables[i], (size_t)n_old * per_key, hipMemcpyDeviceToDevice, s));
            }
            HIP_TRY(hipMemcpyAsync(J.now.on_curve, J.old.on_curve, n_old, hipMemcpyDeviceToDevice, s));
            J.now.lookup = region + s_new; J.now.lookup_mask = s_new - 1;
            if (!A.rebuild) HIP_TRY(hipMemcpyAsync(J.now.lookup, J.old.lookup, (size_t)s_old * 4, hipMemcpyDeviceToDevice, s));
        } else {
            J.now = J.old;
            if (n_add) {
                // the words block of the new size: the next of the last side allocation, or the first of a new one
                if (J.side_back && J.word_blocks < KEYSET_WORD_BLOCKS) {
                    J.now.words = reinterpret_cast<uint32_t*>(J.side_back + 256 * (size_t)J.word_blocks);
                } else {
                    if (int e = keyset_grow_alloc(J.fresh_side, 256 * (size_t)KEYSET_WORD_BLOCKS, "a key set's size words")) return e;
                    J.now.words = reinterpret_cast<uint32_t*>(J.fresh_side.get());
                }
                J.took_block = true;
            }
            if (A.rebuild) {               // beside the live table: the region's base is the live table's address less its slot count
                if (2ull * s_new > J.old.lookup_room) return fail(JJS_ERR_HIP, "the key set's lookup region (%u slots) does not hold a table of %u", J.old.lookup_room, s_new);
                J.now.lookup = J.old.lookup - s_old + s_new; J.now.lookup_mask = s_new - 1;
            }
        }
        if (moving || n_add) HIP_TRY(hipMemcpyAsync(J.now.words, words, sizeof(words), hipMemcpyHostToDevice, s));
        if (n_add) {
            const size_t base_bytes = pad256((size_t)n_add * kt_positions(w) * KT_BASE_WORDS * 4), valid_bytes = pad256(((size_t)n_add + 1) * 4);
            const size_t item_bytes = pad256((size_t)n_add * 4), bad_bytes = pad256(n_add);
            if (int e = keyset_grow_alloc(J.tmp_b, 256 + item_bytes + bad_bytes + cols * (base_bytes + valid_bytes), "a key set's build area")) return e;
            uint8_t* q = J.tmp_b;
            uint32_t* k_counters = reinterpret_cast<uint32_t*>(q); q += 256;
            uint32_t* key_item = reinterpret_cast<uint32_t*>(q); q += item_bytes;
            uint8_t* bad_new = q; q += bad_bytes;
            // the key-table path's own kernels over the new range only: a key_params whose columns start at n_old
            key_params K{};
            K.n_cols = cols; K.max_keys = n_add; K.max_keys_wide = n_add; K.quad_chains = 1; K.n = n_add; K.counters = k_counters;
            for (uint32_t i = 0; i < cols; ++i) {
                key_column& C = K.col[i];
                C.src = fe_src{J.now.keys[i] + (size_t)n_old * 64, 64, 0};
                C.key_item = key_item;
                C.key_flags = J.now.flags[i] + n_old;
                C.bases = reinterpret_cast<uint32_t*>(q); q += base_bytes;
                C.valid_ids = reinterpret_cast<uint32_t*>(q); q += valid_bytes;
                C.tables = J.now.tables[i] + (size_t)n_old * (per_key / 4);
            }
            HIP_TRY(hipMemcpyAsync(key_item, ids.data(), (size_t)n_add * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(k_counters, counters, sizeof(counters), hipMemcpyHostToDevice, s));
            for (uint32_t i = 0; i < cols; ++i)
                HIP_TRY(hipMemsetAsync(J.now.tables[i] + (size_t)n_old * (per_key / 4), 0, (size_t)n_add * per_key, s));      // invalid keys get no tables
            if (unique) {
                HIP_TRY(hipMemsetAsync(bad_new, 0, bad_bytes, s));          // (a candidate that was `bad` is malformed: not among them)
                for (uint32_t i = 0; i < cols; ++i) J.P.dst[i] = J.now.keys[i] + (size_t)n_old * 64;
                hipLaunchKernelGGL(keyset_add_gather_kernel, dim3((A.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, J.P);
            } else {
                for (uint32_t i = 0; i < cols; ++i)
                    HIP_TRY(hipMemcpyAsync(J.now.keys[i] + (size_t)n_old * 64, J.cand[i], (size_t)n_add * 64, hipMemcpyDeviceToDevice, s));
                HIP_TRY(hipMemcpyAsync(bad_new, J.bad, n_add, hipMemcpyDeviceToDevice, s));
            }
            hipLaunchKernelGGL(key_chain_kernel, dim3((unsigned)((5ull * cols * n_add + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, K);
            hipLaunchKernelGGL(keyset_flags_kernel, dim3((n_add + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, J.now.flags[0] + n_old,
                               cols > 1 ? J.now.flags[1] + n_old : nullptr, (const uint8_t*)bad_new, n_add);
            hipLaunchKernelGGL(key_table_kernel, dim3((unsigned)(((uint64_t)cols * n_add * KT_MAX_POSITIONS + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, K);
            HIP_TRY(hipGetLastError());
            for (uint32_t i = 0; i < cols; ++i)
                HIP_TRY(hipMemcpyAsync(flags_out + (size_t)i * n_add, J.now.flags[i] + n_old, n_add, hipMemcpyDeviceToHost, s));
        }
        if (unique && A.n) {
            hipLaunchKernelGGL(keyset_add_answer_kernel, dim3((A.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, J.P, (const uint8_t*)J.now.flags[0],
                               (const uint8_t*)J.now.flags[1], J.idx_dev, J.status_dev);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(idx_out, J.idx_dev, (size_t)A.n * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(status_out, J.status_dev, A.n, hipMemcpyDeviceToHost, s));
        }
        // the lookup table last (see the head of this file): the new ids in place, or every id into a table with more slots
        if (n_add) {
            keyset_lookup T{};
            for (uint32_t i = 0; i < cols; ++i) { T.keys[i] = J.now.keys[i]; T.flags[i] = J.now.flags[i]; }
            T.on_curve = J.now.on_curve; T.slots = J.now.lookup; T.mask = J.now.lookup_mask;
            T.n_keys = n_new; T.n_cols = cols; T.seed = A.seed;
            if (A.rebuild) {
                HIP_TRY(hipMemsetAsync(T.slots, 0xFF, (size_t)s_new * 4, s));
                hipLaunchKernelGGL(keyset_lookup_insert_kernel, dim3((n_new + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, T);
            } else {
                J.entered_in_place = !moving;
                hipLaunchKernelGGL(keyset_lookup_insert_range_kernel, dim3((n_add + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, T, n_old);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    }();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

// A growth call that fails after a device entered new ids into its live lookup table takes them out again (ka_retract); the
// set is still registered, so its memory is.  Best effort: a device that cannot run this has failed altogether.
static void keyset_grow_retract(const keyset_grow_call& A, std::vector<std::unique_ptr<keyset_grow_job>>& jobs) {
    device_restore restore;
    for (auto& job : jobs) {
        keyset_grow_job& J = *job;
        if (!J.entered_in_place) continue;
        J.entered_in_place = false;
        if (hipSetDevice(J.dev->device) != hipSuccess) continue;
        const uint32_t n_slots = J.old.lookup_mask + 1;
        hipLaunchKernelGGL(keyset_add_retract_kernel, dim3((n_slots + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)J.s, J.old.lookup, n_slots, A.n_old);
        (void)hipStreamSynchronize(J.s);
        (void)hipGetLastError();
    }
}

// Leaves a growth call on every way out: the set (if it is still there) may grow again, the call is counted out.
struct keyset_grow_leave {
    jjs_keyset ks;
    ~keyset_grow_leave() {
        std::lock_guard<std::mutex> lock(L.mu);
        if (keyset_entry* k = g_keysets.find(ks)) k->growing = false;
        --g_keyset_grows;
        --g_blocking_calls;
        L.lane_cv.notify_all();
    }
};

// jjs_keyset_add (reserve_total == 0) and jjs_keyset_reserve (n == 0, reserve_total the capacity asked for).
static int keyset_grow(jjs_keyset ks, int format, const uint8_t* keys, const uint8_t* keys2, size_t n, int mode, size_t reserve_total,
                       uint8_t* key_status, uint32_t* idx_out, size_t* n_added) {
    const bool reserve = reserve_total != 0;
    keyset_grow_call A;
    std::vector<device_state*> devs;
    std::vector<std::unique_ptr<keyset_grow_job>> jobs;         // (a job owns a stream: it does not move)
    {
        std::unique_lock<std::mutex> lock(L.mu);
        keyset_entry* k = nullptr;
        for (;;) {
            if (int rc = check_ready()) return rc;
            k = g_keysets.find(ks);
            if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
            if (!k->growing) break;
            L.lane_cv.wait(lock);           // another add or reserve of this set is at work
        }
        if (!reserve) {
            if (format < 0 || format > 2) return fail(JJS_ERR_ARG, "format out of range");
            if (mode != JJS_KEYSET_ADD_APPEND && mode != JJS_KEYSET_ADD_UNIQUE) return fail(JJS_ERR_ARG, "unknown mode");
            if (n == 0) {
                if (n_added) *n_added = 0;
                return JJS_OK;
            }
            if (!keys) return fail(JJS_ERR_ARG, "null key column");
            if (k->n_cols > 1 && format != JJS_FORMAT_WIRE && !keys2) return fail(JJS_ERR_ARG, "the second key column is missing");
            if (n > KEYSET_MAX_KEYS || (size_t)k->n_keys + n > KEYSET_MAX_KEYS) return fail(JJS_ERR_ARG, "a key set holds at most 2^24 keys");
        } else {
            if (reserve_total > KEYSET_MAX_KEYS) return fail(JJS_ERR_ARG, "a key set holds at most 2^24 keys");
            if (reserve_total <= k->capacity) return JJS_OK;
        }
        A.scheme = k->scheme; A.format = format; A.mode = mode; A.cols = k->n_cols; A.n_old = k->n_keys; A.cap = k->capacity;
        A.n = (uint32_t)n; A.seed = k->lookup_seed; A.src[0] = keys; A.src[1] = keys2;
        if (int rc = no_throw([&] {
                devs = L.devs;
                for (size_t i = 0; i < k->copies.size(); ++i) jobs.emplace_back(new keyset_grow_job());
                return k->copies.size() == devs.size() ? (int)JJS_OK : fail(JJS_ERR_NOT_INIT, "the key set was built for other devices");
            }))
            return rc;
        for (size_t i = 0; i < jobs.size(); ++i) {
            const keyset_copy& c = k->copies[i];
            jobs[i]->dev = c.dev;
            jobs[i]->old = static_cast<const keyset_regions&>(c);
            jobs[i]->side_back = c.side.empty() ? nullptr : c.side.back().get();
            jobs[i]->word_blocks = c.word_blocks;
        }
        k->growing = true;
        ++g_blocking_calls;
        ++g_keyset_grows;
    }
    keyset_grow_leave leave_on_every_way_out{ks};
    std::vector<uint8_t> flags, status;         // of the first copy: every device computes the same
    std::vector<uint32_t> idx;
    const int rc = no_throw([&]() -> int {
        device_restore restore;
        // stage A on every device, then -- the number of new keys known -- what the copies have to become, then stage B
        for (auto& job : jobs) {
            keyset_grow_job& J = *job;
            g = J.dev;
            HIP_TRY(hipSetDevice(J.dev->device));
            HIP_TRY(J.s.create(hipStreamNonBlocking));
            if (reserve) continue;
            uint32_t n_first = 0;
            if (int e = keyset_grow_plan(A, J, &n_first)) return e;
            if (&J != jobs[0].get() && n_first != A.n_add) return fail(JJS_ERR_HIP, "the devices disagree about the new keys");
            A.n_add = n_first;
        }
        A.n_new = A.n_old + A.n_add;
        const uint32_t needed = reserve ? (uint32_t)reserve_total : A.n_new;
        A.new_cap = A.cap;
        if (needed > A.cap) {
            const uint64_t half = (uint64_t)A.cap + A.cap / 2;
            A.new_cap = reserve ? needed : (uint32_t)(half > needed ? (half > KEYSET_MAX_KEYS ? KEYSET_MAX_KEYS : half) : needed);
        }
        A.rebuild = kl_slot_count(A.n_new) != jobs[0]->old.lookup_mask + 1;
        flags.resize((size_t)A.cols * A.n_add);
        idx.resize(A.n); status.resize(A.n);
        for (auto& job : jobs) {
            keyset_grow_job& J = *job;
            g = J.dev;
            HIP_TRY(hipSetDevice(J.dev->device));
            const bool first = &J == jobs[0].get();
            std::vector<uint8_t> f(first ? 0 : flags.size()), st(first ? 0 : status.size());
            std::vector<uint32_t> ix(first ? 0 : idx.size());
            if (int e = keyset_grow_build(A, J, first ? flags.data() : f.data(), first ? idx.data() : ix.data(), first ? status.data() : st.data())) return e;
            J.tmp_a = device_mem<uint8_t>(); J.tmp_b = device_mem<uint8_t>();       // (their stream is drained)
        }
        return JJS_OK;
    });
    if (rc) {                   // (nothing was published; what was allocated is freed with `jobs`: every stream is drained)
        keyset_grow_retract(A, jobs);
        return rc;
    }
    uint32_t valid = 0, known = 0;
    for (uint32_t i = 0; i < A.n_add; ++i) {
        const uint32_t st = ks_key_status(flags[i], A.cols > 1 ? flags[(size_t)A.n_add + i] : (uint32_t)KT_KEY_VALID);
        valid += st == ST_OK;
        if (mode == JJS_KEYSET_ADD_APPEND && !reserve) { status[i] = (uint8_t)st; idx[i] = A.n_old + i; }
    }
    if (mode == JJS_KEYSET_ADD_UNIQUE)
        for (uint32_t i = 0; i < A.n; ++i) known += idx[i] < A.n_old;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        keyset_entry* k = g_keysets.find(ks);
        if (!k) return fail(JJS_ERR_ARG, "the key set was destroyed during the call");
        if (L.devs != devs || k->copies.size() != jobs.size()) {
            keyset_grow_retract(A, jobs);
            return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
        }
        const bool moving = A.new_cap != A.cap;
        if (int prc = no_throw([&] {
                for (keyset_copy& c : k->copies) c.side.reserve(c.side.size() + 1);
                return JJS_OK;
            })) {
            keyset_grow_retract(A, jobs);
            return prc;
        }
        device_state* const keep = g;
        for (size_t i = 0; i < jobs.size(); ++i) {
            keyset_copy& c = k->copies[i];
            keyset_grow_job& J = *jobs[i];
            static_cast<keyset_regions&>(c) = J.now;
            if (moving) {              // launches already queued still read the old allocation: retired, as a destroyed set's
                g = c.dev;
                c.mem.replace(std::move(J.fresh));
                for (auto& m : c.side) m.release();
                c.side.clear();
                c.word_blocks = 0;
            } else if (J.took_block) {
                if (J.fresh_side) { c.side.push_back(std::move(J.fresh_side)); c.word_blocks = 1; }
                else ++c.word_blocks;
            }
        }
        g = keep;
        k->n_keys = A.n_new; k->valid += valid; k->capacity = A.new_cap;
        if (!reserve) { ++k->growth[JJS_KEYSET_ADD_CALLS]; k->growth[JJS_KEYSET_ADD_KNOWN] += known; }
        if (moving) ++k->growth[JJS_KEYSET_RELOCATIONS];
        if (A.rebuild) ++k->growth[JJS_KEYSET_LOOKUP_REBUILDS];
    }
    if (!reserve) {
        if (key_status) memcpy(key_status, status.data(), A.n);
        if (idx_out) memcpy(idx_out, idx.data(), (size_t)A.n * 4);
        if (n_added) *n_added = A.n_add;
    }
    return JJS_OK;
}
}  // extern "C++"

extern "C" {

int jjs_keyset_add(jjs_keyset ks, int format, const uint8_t* keys, const uint8_t* keys2, size_t n, int mode, uint8_t* key_status,
                   uint32_t* idx_out, size_t* n_added) {
    return keyset_grow(ks, format, keys, keys2, n, mode, 0, key_status, idx_out, n_added);
}

int jjs_keyset_reserve(jjs_keyset ks, size_t n_keys_total) {
    if (n_keys_total == 0) {               // every set has that much: only the handle is looked at
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        return g_keysets.find(ks) ? (int)JJS_OK : fail(JJS_ERR_ARG, "unknown or destroyed key set");
    }
    return keyset_grow(ks, 0, nullptr, nullptr, 0, 0, n_keys_total, nullptr, nullptr, nullptr);
}

int jjs_keyset_growth(jjs_keyset ks, uint64_t out[JJS_KEYSET_GROWTH]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = g_keysets.find(ks);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    for (int i = 0; i < JJS_KEYSET_GROWTH; ++i) out[i] = k->growth[i];
    out[JJS_KEYSET_CAPACITY] = k->capacity;
    return JJS_OK;
}

}  // extern "C"

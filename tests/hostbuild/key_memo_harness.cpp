// CPU build of the key-table path WITH the memo of the slot's last call (csrc/key_tables.h step 5) for
// tests/test_key_memo_host.py: a "slot" owns a pool of bases and tables and a memo, both of which outlive a call; a call
// runs the dedup (std::map, as host_harness.cpp), the match and place steps through the product's own per-key functions
// (kt_memo_match, kt_memo_free, kt_memo_claim, kt_memo_insert) in the order and with the modes of the device's kernels
// (device_kernels.h key_match_kernel / key_place_kernel, verify_job.h setup_keys), builds what missed and verifies every
// item with kt_finish_item.  The pool starts as garbage and is never cleared: a key that is taken for another one, or found
// after its tables were overwritten, reads the wrong tables and gets the wrong statuses.
// The comb tables and the double scheme's tag come from host_harness.cpp.
#include "host_harness.cpp"

namespace {
struct memo_column {
    std::vector<uint32_t> bases, tables, key, stamp, pool_of, todo, hit, hdr;
    std::vector<unsigned long long> hash;
    std::vector<uint8_t> flags;
};
struct memo_slot {
    uint32_t cap = 0;
    uint64_t seed = 0x5eed5eed12345678ull;
    uint32_t call = 0, cols = 0;
    bool flush = true;
    memo_column col[2];
    void fresh() {               // a new pool: what ensure_key_pool / jjs_trim leave
        for (memo_column& c : col) {
            c.bases.assign((size_t)cap * KT_MAX_POSITIONS * KT_BASE_WORDS + 4, 0xDEADBEEFu);
            c.tables.assign(kt_table_words_for_keys(cap, cap) + 8, 0xA5C3F00Du);
            size_t slots = 64;
            while (slots < 2 * (size_t)cap) slots <<= 1;
            c.hash.assign(slots, 0);
            c.key.assign((size_t)cap * 16, 0); c.stamp.assign(cap + 1, 0); c.pool_of.assign(cap + 1, 0);
            c.todo.assign(cap + 1, 0); c.hit.assign(cap + 1, 0); c.hdr.assign(64, 0); c.flags.assign(cap + 1, 0);
        }
        flush = true;
    }
};
}  // namespace

extern "C" {

void* jjs_memo_host_new(uint32_t cap) {
    memo_slot* s = new memo_slot;
    s->cap = cap;
    s->fresh();
    return s;
}
void jjs_memo_host_free(void* slot) { delete static_cast<memo_slot*>(slot); }
void jjs_memo_host_new_pool(void* slot) { static_cast<memo_slot*>(slot)->fresh(); }

// One call in the slot.  scheme 0 / 1 / 2 with the columns of the scheme (Rp, K2 NULL where it has none: K2 = PK' or Gen);
// window 5 or 6 = the decision of the device, 0 = the batch turns the tables down (nothing is verified then: status untouched);
// off != 0: KT_MEMO_OFF (a wire call).  counts: hits of column 0, 1, built keys of column 0, 1.  Returns 0, or -2 when the
// distinct keys do not fit the pool.
int jjs_memo_host_call(void* slot, int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK,
                       const uint8_t* K2, const uint8_t* m, size_t n, int window, int off, uint8_t* status, uint32_t counts[4]) {
    memo_slot& S = *static_cast<memo_slot*>(slot);
    if (scheme < 0 || scheme > 2 || (window != 0 && window != KT_WINDOW_NARROW && window != KT_WINDOW_WIDE)) return -1;
    ensure_tables();
    const out_ptrs o{status, nullptr, nullptr, nullptr};
    verify_params P = scheme == 0 ? params_single(u, R, PK, m, n, g_comb_g.data(), o)
                    : scheme == 1 ? params_double(u, R, Rp, PK, K2, m, n, (const uint8_t*)g_tag, g_comb_g.data(), g_comb_gn.data(), o)
                                  : params_vargen(u, R, PK, K2, m, n, o);
    key_params K{};
    K.n = n; K.max_keys = S.cap; K.max_keys_wide = S.cap; K.pool_cap = S.cap;
    fe_src cols[2];
    for (uint32_t e = 0; e < P.n_eq; ++e) {
        cols[P.eq[e].pk_col] = P.eq[e].pk; K.n_cols = std::max(K.n_cols, (uint32_t)P.eq[e].pk_col + 1);
        if (!P.eq[e].comb) { cols[P.eq[e].gen_col] = P.eq[e].gen; K.n_cols = std::max(K.n_cols, (uint32_t)P.eq[e].gen_col + 1); }
    }
    std::vector<uint32_t> counters(64, 0), keyid[2], key_item[2], valid_ids[2];
    std::vector<uint8_t> flags[2];
    K.counters = counters.data();
    for (uint32_t c = 0; c < K.n_cols; ++c) {
        key_column& C = K.col[c];
        memo_column& MC = S.col[c];
        C.src = cols[c];
        keyid[c].resize(n + 1);
        std::map<std::string, uint32_t> seen;
        for (uint64_t i = 0; i < n; ++i) {
            std::string key((const char*)(C.src.base + i * C.src.stride + C.src.off), 64);
            auto it = seen.find(key);
            if (it == seen.end()) { it = seen.emplace(key, (uint32_t)seen.size()).first; key_item[c].push_back((uint32_t)i); }
            keyid[c][i] = it->second;
        }
        counters[c] = (uint32_t)key_item[c].size();
        if (counters[c] > S.cap) return -2;
        flags[c].assign(counters[c] + 1, 0); valid_ids[c].assign(counters[c] + 1, 0);
        C.keyid = keyid[c].data(); C.key_item = key_item[c].data(); C.key_flags = flags[c].data(); C.valid_ids = valid_ids[c].data();
        C.bases = MC.bases.data();
        C.tables = (uint32_t*)(((uintptr_t)MC.tables.data() + 15) & ~(uintptr_t)15);
        C.pool_of = MC.pool_of.data();
        key_memo& M = K.memo[c];
        M.hash = MC.hash.data(); M.hash_mask = (uint32_t)(MC.hash.size() - 1); M.cap = S.cap; M.key = MC.key.data();
        M.flags = MC.flags.data(); M.stamp = MC.stamp.data(); M.todo = MC.todo.data(); M.hit = MC.hit.data(); M.hdr = MC.hdr.data();
    }
    // setup_keys
    K.memo_seed = S.seed;
    if (++S.call == 0) S.call = 1;
    K.memo_call = S.call;
    K.memo_mode = S.flush || S.cols != K.n_cols ? KT_MEMO_FLUSH : KT_MEMO_LIVE;
    if (off) K.memo_mode = KT_MEMO_OFF;
    S.flush = false; S.cols = K.n_cols;
    counters[2] = (uint32_t)window;
    const uint32_t w = counters[2];
    // key_match_kernel
    for (uint32_t c = 0; c < K.n_cols; ++c) {
        const key_column C = kt_col(K, (int32_t)c);
        const key_memo M = kt_memo(K, (int32_t)c);
        if (!w || K.memo_mode == KT_MEMO_OFF) {
            const uint32_t none = 0u;
            M.hdr[0] = none;
            if (!w) continue;
            for (uint32_t id = 0; id < counters[c]; ++id) { C.pool_of[id] = id; M.todo[counters[8 + c]++] = id; }
            continue;
        }
        const bool live = K.memo_mode == KT_MEMO_LIVE && M.hdr[0] == w;
        for (uint32_t id = 0; id < counters[c]; ++id) {
            if (kt_memo_match(C, M, id, live, K.memo_seed, K.memo_call)) ++counters[12 + c];
            else M.todo[counters[8 + c]++] = id;
        }
    }
    if (counts) { counts[0] = counters[12]; counts[1] = counters[13]; counts[2] = counters[8]; counts[3] = counters[9]; }
    if (!w) return 0;
    // key_place_kernel
    if (K.memo_mode != KT_MEMO_OFF)
        for (uint32_t c = 0; c < K.n_cols; ++c) {
            const key_column C = kt_col(K, (int32_t)c);
            const key_memo M = kt_memo(K, (int32_t)c);
            for (uint32_t p = 0; p < K.pool_cap && counters[10 + c] < counters[8 + c]; ++p)
                if (kt_memo_free(M, p, K.memo_call)) kt_memo_claim(C, M, M.todo[counters[10 + c]++], p, K.memo_seed, K.memo_call);
            if (counters[10 + c] != counters[8 + c]) return -3;           // cannot happen: the keys fit the pool
            for (uint32_t id = 0; id < counters[c]; ++id)
                if (M.hit[id] != KT_MEMO_NONE) kt_memo_insert(C, M, id, M.hit[id], K.memo_seed, K.memo_call);
            M.hdr[0] = w; M.hdr[1] = K.memo_call;
        }
    // key_chain_kernel, key_table_kernel: the todo list, and its valid members
    for (uint32_t c = 0; c < K.n_cols; ++c) {
        const key_column C = kt_col(K, (int32_t)c);
        const key_memo M = kt_memo(K, (int32_t)c);
        for (uint32_t j = 0; j < counters[8 + c]; ++j) {
            const uint32_t id = M.todo[j];
            const bool valid = kt_chain_key(C, id, (int)w);
            kt_memo_flags(C, M, id);
            if (valid) C.valid_ids[counters[5 + c]++] = id;
        }
        for (uint32_t j = 0; j < counters[5 + c]; ++j)
            for (uint32_t pos = 0; pos < (uint32_t)kt_positions((int)w); ++pos) kt_table_lane(C, C.valid_ids[j], pos, (int)w);
    }
    P.key_flag = &counters[2];
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t st = kt_finish_item(P, K, i, prepare_item(P, i));
        if (st >= ST_PENDING_EQ_FAILED) st = resolve_item(P, i, st == ST_PENDING_EQ_HELD);
        status[i] = (uint8_t)st;
    }
    return 0;
}
// the pool index of every distinct key of column c in the order of first appearance is not exposed: the tests see the memo
// through the hit / built counts and through the statuses
}  // extern "C"

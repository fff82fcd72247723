// CPU build of csrc/keyset_remove.h (removing keys from a live key set, compacting it) for tests/test_keyset_remove_host.py:
// the JJS_HD stage bodies the device runs -- answer, flags, retract, re-enter; mark, the add's scan, gather, the table gather --
// in the order and the decomposition of the device's launches, the lanes of a launch one after the other (forwards or
// backwards).  A session holds one set, as a device copy holds it: rows, flag bytes, on-curve bytes, window tables (optional,
// filled with a pattern: nothing here reads them as points) and the lookup table; adds that follow a remove run the real probe
// and insert of keyset_lookup.h over it.
#include "keyset_add_harness.cpp"
#include "keyset_remove.h"

namespace {

struct kr_session {
    uint32_t cols = 0, n = 0, cap = 0, units = 0;
    uint64_t seed = 0;
    aligned_rows rows[2];
    std::vector<uint32_t> flags[2];           // the flag bytes, in words: kr_mark_byte addresses the aligned word
    std::vector<uint8_t> on_curve;
    std::vector<kr_unit> tables[2];           // cap x units, or empty
    std::vector<uint32_t> slots;
    uint8_t* flag_bytes(uint32_t c) { return reinterpret_cast<uint8_t*>(flags[c].data()); }
    keyset_lookup lookup() {
        keyset_lookup T{};
        for (uint32_t c = 0; c < cols; ++c) { T.keys[c] = rows[c].p; T.flags[c] = flag_bytes(c); }
        T.on_curve = on_curve.data(); T.slots = slots.data(); T.mask = (uint32_t)slots.size() - 1;
        T.n_keys = n; T.n_cols = cols; T.seed = seed;
        return T;
    }
    void rebuild() {                          // a table of kl_slot_count(n) slots from empty: removed ids are malformed, so skipped
        slots.assign(kl_slot_count(n), KL_EMPTY);
        const keyset_lookup T = lookup();
        for (uint32_t i = 0; i < n; ++i) kl_insert(T, i);
    }
};

// the pattern word w of 16-byte unit u of key `id`'s table in column c (the id the key had when the session was made)
uint32_t pattern(uint32_t c, uint32_t id, uint32_t u, uint32_t w) { return (id * 2654435761u) ^ (c * 0x9e3779b9u) ^ (u * 40503u + w * 7u + (u >> 7)); }

}  // namespace

extern "C" {

uint32_t jjs_kr_table_units(void) { return (uint32_t)((size_t)kt_positions(KEYSET_WINDOW) * kt_table_words(KEYSET_WINDOW) * 4 / 16); }
uint32_t jjs_kr_pattern(uint32_t c, uint32_t id, uint32_t u, uint32_t w) { return pattern(c, id, u, w); }

// rows0, rows1: n x 64; flags0, flags1: the KT_KEY_* byte of each key's points; cap >= n: room for the adds that follow
void* jjs_kr_new(uint32_t n_cols, const uint8_t* rows0, const uint8_t* rows1, const uint8_t* flags0, const uint8_t* flags1, uint32_t n,
                 uint32_t cap, uint64_t seed, int with_tables) {
    if (n_cols < 1 || n_cols > 2 || n == 0 || cap < n) return nullptr;
    kr_session* S = new kr_session();
    S->cols = n_cols; S->n = n; S->cap = cap; S->seed = seed;
    S->units = jjs_kr_table_units();
    const uint8_t *rows[2] = {rows0, rows1}, *flags[2] = {flags0, flags1};
    for (uint32_t c = 0; c < n_cols; ++c) {
        S->rows[c].size(cap);
        memcpy(S->rows[c].p, rows[c], (size_t)n * 64);
        S->flags[c].assign((cap + 3) / 4 + 1, 0);
        memcpy(S->flag_bytes(c), flags[c], n);
        if (with_tables) {
            S->tables[c].resize((size_t)n * S->units);
            for (uint32_t id = 0; id < n; ++id)
                for (uint32_t u = 0; u < S->units; ++u)
                    for (uint32_t w = 0; w < 4; ++w) S->tables[c][(size_t)id * S->units + u][w] = pattern(c, id, u, w);
        }
    }
    S->on_curve.assign(cap, 0xAA);
    S->rebuild();
    return S;
}
void jjs_kr_free(void* h) { delete (kr_session*)h; }
uint32_t jjs_kr_keys(void* h) { return ((kr_session*)h)->n; }
uint32_t jjs_kr_slot_count(void* h) { return (uint32_t)((kr_session*)h)->slots.size(); }

// jjs_keyset_remove's four launches; counts[2] as keyset_remove_plan::counts
int jjs_kr_remove(void* h, const uint32_t* idx, uint32_t n, uint8_t* result, uint32_t* counts, int backwards) {
    kr_session& S = *(kr_session*)h;
    keyset_remove_plan P{};
    P.T = S.lookup();
    P.flags[0] = S.flag_bytes(0); P.flags[1] = S.cols > 1 ? S.flag_bytes(1) : nullptr;
    P.idx = idx; P.result = result; P.counts = counts; P.n = n;
    counts[0] = counts[1] = 0;
    const auto lanes = [&](uint32_t count, auto body) {
        for (uint32_t i = 0; i < count; ++i) body(backwards ? count - 1 - i : i);
    };
    lanes(n, [&](uint32_t i) { kr_answer(P, i); });
    lanes(n, [&](uint32_t i) { kr_flags(P, i); });
    lanes(n, [&](uint32_t i) { kr_retract(P, i); });
    lanes(S.n, [&](uint32_t id) { kr_reenter(P.T, id); });
    return 0;
}

// the probe of n affine rows over the live table
void jjs_kr_find(void* h, const uint8_t* q0, const uint8_t* q1, uint32_t n, uint32_t* idx_out) {
    kr_session& S = *(kr_session*)h;
    const keyset_lookup T = S.lookup();
    aligned_rows q[2];
    const uint8_t* src[2] = {q0, q1};
    for (uint32_t c = 0; c < S.cols; ++c) { q[c].size(n); memcpy(q[c].p, src[c], (size_t)n * 64); }
    for (uint32_t i = 0; i < n; ++i) idx_out[i] = kl_find_item(T, false, q[0].p, q[1].p, i);
}

// flags_out [cols][n] and slots_out [slot count]
void jjs_kr_state(void* h, uint8_t* flags_out, uint32_t* slots_out, uint8_t* rows_out) {
    kr_session& S = *(kr_session*)h;
    for (uint32_t c = 0; c < S.cols; ++c) {
        memcpy(flags_out + (size_t)c * S.n, S.flag_bytes(c), S.n);
        if (rows_out) memcpy(rows_out + (size_t)c * S.n * 64, S.rows[c].p, (size_t)S.n * 64);
    }
    memcpy(slots_out, S.slots.data(), S.slots.size() * 4);
}

// A later add of n rows with the flag bytes they get: appended (the new ids entered in place, or every id into a table with
// more slots), or unique: a row the live table finds is answered with that index, a malformed one with KA_MALFORMED, any other
// is registered -- one candidate after the other, which gives the indices of the device's plan (first occurrences in order).
int jjs_kr_add(void* h, const uint8_t* rows0, const uint8_t* rows1, const uint8_t* flags0, const uint8_t* flags1, uint32_t n, int unique,
               uint32_t* idx_out) {
    kr_session& S = *(kr_session*)h;
    if (S.n + n > S.cap || !S.tables[0].empty()) return -1;
    const uint8_t *rows[2] = {rows0, rows1}, *flags[2] = {flags0, flags1};
    for (uint32_t i = 0; i < n; ++i) {
        const bool malformed = ((flags0[i] | (S.cols > 1 ? flags1[i] : 0)) & KT_KEY_MALFORMED) != 0;
        const uint32_t id = S.n;
        for (uint32_t c = 0; c < S.cols; ++c) {           // (beyond n_keys: nothing reads the row until the id is counted in)
            memcpy(S.rows[c].p + (size_t)id * 64, rows[c] + (size_t)i * 64, 64);
            S.flag_bytes(c)[id] = flags[c][i];
        }
        if (unique) {
            if (malformed) { idx_out[i] = KA_MALFORMED; continue; }
            keyset_lookup T = S.lookup();
            T.n_keys = id + 1;                             // (so that the candidate's own row can be loaded: it is in no slot)
            const uint32_t hit = kl_find_affine(T, kl_load_row(T, id));
            if (hit != KL_MISS) { idx_out[i] = hit; continue; }
        }
        idx_out[i] = id;
        S.n = id + 1;
        if (kl_slot_count(S.n) != S.slots.size()) S.rebuild();
        else kl_insert(S.lookup(), id);
    }
    return 0;
}

// jjs_keyset_compact's launches: mark per block of KA_BLOCK ids, the add's scan, the gather by rank, the table gather block by
// block with KA_BLOCK lanes each, the lookup table from empty.  The session becomes the compacted set; map_out [old n].
int jjs_kr_compact(void* h, uint32_t* map_out, int backwards) {
    kr_session& S = *(kr_session*)h;
    const uint32_t n = S.n, blocks = (n + KA_BLOCK - 1) / KA_BLOCK;
    kr_session N;
    N.cols = S.cols; N.seed = S.seed; N.units = S.units;
    std::vector<uint32_t> sums(blocks + 1), src(n);
    keyset_compact_plan P{};
    P.n_keys = n; P.n_cols = S.cols; P.sums = sums.data(); P.src = src.data(); P.map = map_out;
    for (uint32_t c = 0; c < S.cols; ++c) { P.keys[c] = S.rows[c].p; P.flags[c] = S.flag_bytes(c); }
    P.on_curve = S.on_curve.data();
    for (uint32_t b = 0; b < blocks; ++b) {
        uint32_t count = 0;
        for (uint32_t id = b * KA_BLOCK; id < n && id < (b + 1) * KA_BLOCK; ++id) count += kc_survives(P, id);
        sums[b] = count;
    }
    jjs_ka_host_scan(sums.data(), blocks);
    const uint32_t n_new = sums[blocks];
    if (n_new == 0) return -1;
    N.n = n_new; N.cap = n_new;
    for (uint32_t c = 0; c < S.cols; ++c) {
        N.rows[c].size(n_new);
        N.flags[c].assign((n_new + 3) / 4 + 1, 0);
        P.new_keys[c] = N.rows[c].p; P.new_flags[c] = N.flag_bytes(c);
    }
    N.on_curve.assign(n_new, 0x55);
    P.new_on_curve = N.on_curve.data();
    for (uint32_t k = 0; k < blocks; ++k) {
        const uint32_t b = backwards ? blocks - 1 - k : k;
        uint32_t r = sums[b];
        for (uint32_t id = b * KA_BLOCK; id < n && id < (b + 1) * KA_BLOCK; ++id) {
            if (kc_survives(P, id)) kc_gather(P, id, r++);
            else map_out[id] = KR_GONE;
        }
    }
    if (!S.tables[0].empty()) {
        keyset_table_gather G{};
        for (uint32_t c = 0; c < S.cols; ++c) {
            N.tables[c].assign((size_t)n_new * S.units, kr_unit{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu});
            G.old_tables[c] = reinterpret_cast<const uint32_t*>(S.tables[c].data());
            G.new_tables[c] = reinterpret_cast<uint32_t*>(N.tables[c].data());
        }
        G.src = src.data(); G.n_new = n_new; G.n_cols = S.cols; G.units = S.units;
        G.slices = (G.units + KR_TABLE_SLICE - 1) / KR_TABLE_SLICE;
        const uint64_t pieces = (uint64_t)G.slices * n_new * S.cols;
        for (uint64_t k = 0; k < pieces; ++k)
            for (uint32_t lane = 0; lane < KA_BLOCK; ++lane) kc_table_piece(G, backwards ? pieces - 1 - k : k, lane, KA_BLOCK);
    }
    N.rebuild();
    // (kl_insert has written the on-curve bytes again: they must be the gathered ones)
    S = std::move(N);
    return (int)n_new;
}

// the 4 x units words of key `id`'s table in column c
int jjs_kr_table(void* h, uint32_t c, uint32_t id, uint32_t* out) {
    kr_session& S = *(kr_session*)h;
    if (c >= S.cols || id >= S.n || S.tables[c].empty()) return -1;
    memcpy(out, &S.tables[c][(size_t)id * S.units], (size_t)S.units * 16);
    return 0;
}

}  // extern "C"

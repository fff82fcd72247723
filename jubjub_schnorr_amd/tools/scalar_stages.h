// The scalar multiplications of csrc/*.h, one stage per function group, with caller-chosen scalars and points: the comb
// (comb_mul), the per-lane window table (build_point_table + table_mul), the two equations of check_equation, the key tables
// (kt_chain_key, kt_build_table, kt_add_scalar, kt_add_challenge), the latency path (sb_chain_lane, sb_piece and the sum in the order of the
// shuffle tree) and, on the device only, the quad chains (kt_chain_key_quad, sb_chain_lane_quad).  ONE copy of the stage
// bodies and of the record format, compiled into tests/hostbuild/host_harness.cpp (CPU build) and tools/scalarcheck.hip
// (device): the two cannot drift.  The stages only execute; tests/scalar_mul_cases.py writes the inputs and checks every
// output against the Python oracle's big-integer curve arithmetic.
//
//   records:  uint32 code, uint32 count, count * Stage::IN uint32      code = kind << 24 | parameter (window width / positions)
//   output:   per record, count * Stage::OUT uint32
// A stage reads its item at `in` (16-byte aligned, IN a multiple of 4 words: the product's loaders read 16 bytes at a time),
// writes `out` and may use SCRATCH words of 16-byte aligned scratch of its own.  LANES adjacent lanes run one item.
#pragma once
#include <vector>

#include "sign_core.h"
#include "small_batch.h"
#include "key_tables.h"

namespace jjs {
namespace sc {

// the test reads this enum
enum Kind : uint32_t { K_COMB = 1, K_TABLE, K_EQ, K_KT, K_KT_DUMP, K_SB, K_SB_TABLES, K_KT_BASES_QUAD, K_SB_TABLES_QUAD, K_KT_CHALLENGE };
constexpr uint32_t code(uint32_t kind, uint32_t param = 0) { return kind << 24 | param; }

struct ctx {
    const uint32_t* comb[2];      // the comb tables of G and G'
};

JJS_HD words8 ld8(const uint32_t* p) {
    words8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = p[i];
    return r;
}
JJS_HD void st_pt(uint32_t* o, const ext_pt& p) {
    for (int i = 0; i < 9; ++i) { o[i] = p.x.l[i]; o[9 + i] = p.y.l[i]; o[18 + i] = p.z.l[i]; o[27 + i] = p.t.l[i]; }
}
JJS_HD fe_src at(const uint32_t* in, uint32_t word) { return fe_src{reinterpret_cast<const uint8_t*>(in), 0, 4 * word}; }

// k (8) | which (1) | pad (3)  ->  k * G or k * G' (T not valid)
struct Comb {
    static constexpr int LANES = 1, IN = 12, OUT = 36, SCRATCH = 0;
    JJS_HD static void run(const ctx& C, const uint32_t* in, uint32_t* out, uint32_t*, uint32_t) {
        st_pt(out, comb_mul((in[8] & 1u) ? C.comb[1] : C.comb[0], ld8(in)));
    }
};
// P (16) | k (8)  ->  k * P through the lane's window table (T valid)
struct Table {
    static constexpr int LANES = 1, IN = 24, OUT = 36, SCRATCH = TABLE_WORDS;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t) {
        build_point_table(scratch, load_fq(at(in, 0), 0), load_fq(at(in, 0), 0, 32));
        st_pt(out, table_mul(scratch, ld8(in + 16), true));
    }
};

// the item of the equation stages: u (8) | c (8) | PK (16) | R (16) | Gen (16) | mode (1) | pad (3)
// mode 0: fixed generator G, 1: fixed generator G', 2: per-item generator Gen
constexpr int EQ_IN = 68;
JJS_HD eq_desc eq_of(const ctx& C, const uint32_t* in) {
    const uint32_t mode = in[64];
    eq_desc E{};
    E.comb = mode < 2u ? C.comb[mode] : nullptr;
    E.pk = at(in, 16); E.r = at(in, 32); E.gen = at(in, 48);
    E.pk_col = E.gen_col = -1;
    return E;
}
JJS_HD void st_half(uint32_t* out, const half_scalars& h) {
    out[0] = h.b_neg ? 1u : 0u;
    for (int i = 0; i < 4; ++i) { out[1 + i] = h.a.w[i]; out[5 + i] = h.b.w[i]; }
}
// -> verdict of check_equation (1) | sign of b (1) | a (4) | |b| (4) | b*u mod r (8): the half-size values of a fixed generator
struct Eq {
    static constexpr int LANES = 1, IN = EQ_IN, OUT = 18, SCRATCH = WS_WORDS_PER_LANE;
    JJS_HD static void run(const ctx& C, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t) {
        const eq_desc E = eq_of(C, in);
        const words8 u = load_words(at(in, 0), 0), c = load_words(at(in, 8), 0);
        half_scalars h{};
        if (E.comb) h = half_size_scalars(c);
        out[0] = check_equation(E, 0, scratch, u, c, h) ? 1u : 0u;
        st_half(out + 1, h);
        const words8 bu = E.comb ? half_scalar_times_u(h, u) : words8{};
        for (int i = 0; i < 8; ++i) out[10 + i] = bu.w[i];
    }
};

// the key column of one key held in a stage's own memory: word 0 of `head` is its representative item (0), byte 4 its flags
JJS_HD key_column one_key(const uint32_t* in, uint32_t* head, uint32_t* bases, uint32_t* tables) {
    key_column K{};
    K.src = at(in, 0);
    head[0] = 0u;
    K.key_item = head;
    K.key_flags = reinterpret_cast<uint8_t*>(head + 1);
    K.bases = bases;
    K.tables = tables;
    return K;
}
template <int W>
struct KtSizes {
    static constexpr int BASES = kt_positions(W) * KT_BASE_WORDS, TABLES = kt_positions(W) * kt_table_words(W);
    static_assert(BASES % 4 == 0 && TABLES % 4 == 0, "the tables are stored 16 bytes at a time");
};
// P (16) | s (8)  ->  s * P through the key's tables (36, T valid) | key flags (1) | kt_chain_key's verdict (1)
template <int W>
struct Kt {
    static constexpr int LANES = 1, IN = 24, OUT = 38, SCRATCH = 4 + KtSizes<W>::BASES + KtSizes<W>::TABLES;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t) {
        const key_column K = one_key(in, scratch, scratch + 4, scratch + 4 + KtSizes<W>::BASES);
        const bool valid = kt_chain_key(K, 0, W);
        for (uint32_t pos = 0; pos < (uint32_t)kt_positions(W); ++pos) kt_table_lane(K, 0, pos, W);
        st_pt(out, kt_add_scalar(ext_identity(), K, 0, ld8(in + 16), W));
        out[36] = K.key_flags[0];
        out[37] = valid ? 1u : 0u;
    }
};
// P (16) | c (8), c < 2^250  ->  c * P as kt_finish_item adds a challenge (kt_add_challenge: 36, T valid)
template <int W>
struct KtChallenge {
    static constexpr int LANES = 1, IN = 24, OUT = 36, SCRATCH = 4 + KtSizes<W>::BASES + KtSizes<W>::TABLES;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t) {
        const key_column K = one_key(in, scratch, scratch + 4, scratch + 4 + KtSizes<W>::BASES);
        kt_chain_key(K, 0, W);
        for (uint32_t pos = 0; pos < (uint32_t)kt_positions(W); ++pos) kt_table_lane(K, 0, pos, W);
        st_pt(out, kt_add_challenge(ext_identity(), K, 0, ld8(in + 16), W));
    }
};
// P (16) | pad (8)  ->  the bases 2^(W i) P (positions x 36) | the tables j * base (positions x entries x 36)
template <int W>
struct KtDump {
    static constexpr int LANES = 1, IN = 24, OUT = KtSizes<W>::BASES + KtSizes<W>::TABLES, SCRATCH = 4;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t) {
        const key_column K = one_key(in, scratch, out, out + KtSizes<W>::BASES);
        kt_chain_key(K, 0, W);
        for (uint32_t pos = 0; pos < (uint32_t)kt_positions(W); ++pos) kt_table_lane(K, 0, pos, W);
    }
};

JJS_HD small_params small_of(const ctx& C, const uint32_t* in, uint32_t* tables, uint32_t positions) {
    small_params S{};
    S.V.n_eq = 1; S.V.n = 1; S.V.small_mode = 1;
    S.V.eq[0] = eq_of(C, in);
    S.V.u = at(in, 0);
    S.tables = tables;
    S.positions = positions;
    S.windows = S.V.eq[0].comb ? 32u : 64u;
    return S;
}
// the item of Eq with a prep_record built here  ->  verdict (1) | sign of b, a, |b| (9) | the sum of the pieces (36, T valid)
template <int POS>
struct Sb {
    static constexpr int LANES = 1, IN = EQ_IN, OUT = 46, SCRATCH = 2 * POS * TABLE_WORDS;
    JJS_HD static void run(const ctx& C, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t) {
        const small_params S = small_of(C, in, scratch, POS);
        prep_record r{};
        r.c = load_words(at(in, 8), 0);
        if (S.V.eq[0].comb) r.h = half_size_scalars(r.c);
        for (uint32_t pt = 0; pt < 2; ++pt)
            for (uint32_t k = 0; k < POS; ++k) sb_chain_lane(S, 0, 0, pt, k);
        ext_pt part[POS];
        for (uint32_t k = 0; k < POS; ++k) part[k] = sb_piece(S, 0, 0, k, r);
        for (uint32_t step = 1; step < POS; step <<= 1)                   // the order of sb_verify_item_serial
            for (uint32_t k = 0; k < POS; k += 2 * step) part[k] = sb_add(part[k], part[k + step]);
        out[0] = sb_equation_holds(S, 0, 0, part[0]) ? 1u : 0u;
        st_half(out + 1, r.h);
        st_pt(out + 10, part[0]);
    }
};
// the same item  ->  the window tables of the chain lanes: [PK, R or Gen][position][9 entries x 36]
template <int POS>
struct SbTables {
    static constexpr int LANES = 1, IN = EQ_IN, OUT = 2 * POS * TABLE_WORDS, SCRATCH = 0;
    JJS_HD static void run(const ctx& C, const uint32_t* in, uint32_t* out, uint32_t*, uint32_t) {
        const small_params S = small_of(C, in, out, POS);
        for (uint32_t pt = 0; pt < 2; ++pt)
            for (uint32_t k = 0; k < POS; ++k) sb_chain_lane(S, 0, 0, pt, k);
    }
};
#if defined(__HIPCC__)
// device only: the same bases and the same tables from the chains on four lanes
template <int W>
struct KtBasesQuad {
    static constexpr int LANES = 4, IN = 24, OUT = KtSizes<W>::BASES, SCRATCH = 4;
    __device__ static void run(const ctx&, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t j) {
        const key_column K = one_key(in, scratch, out, nullptr);
        kt_chain_key_quad(K, 0, W, j);
    }
};
template <int POS>
struct SbTablesQuad {
    static constexpr int LANES = 4, IN = EQ_IN, OUT = 2 * POS * TABLE_WORDS, SCRATCH = 0;
    __device__ static void run(const ctx& C, const uint32_t* in, uint32_t* out, uint32_t*, uint32_t j) {
        const small_params S = small_of(C, in, out, POS);
        for (uint32_t pt = 0; pt < 2; ++pt)
            for (uint32_t k = 0; k < POS; ++k) sb_chain_lane_quad(S, 0, 0, pt, k, j);
    }
};
#endif

// One record through executor X, whose step<Stage>(count) runs the stage on every item.  Non-zero: unknown code or X's error.
template <typename X>
int dispatch(X& x, uint32_t c, uint32_t n) {
    switch (c) {
    case code(K_COMB): return x.template step<Comb>(n);
    case code(K_TABLE): return x.template step<Table>(n);
    case code(K_EQ): return x.template step<Eq>(n);
    case code(K_KT, 5): return x.template step<Kt<5>>(n);
    case code(K_KT, 6): return x.template step<Kt<6>>(n);
    case code(K_KT_DUMP, 5): return x.template step<KtDump<5>>(n);
    case code(K_KT_DUMP, 6): return x.template step<KtDump<6>>(n);
    case code(K_KT_CHALLENGE, 5): return x.template step<KtChallenge<5>>(n);
    case code(K_KT_CHALLENGE, 6): return x.template step<KtChallenge<6>>(n);
    case code(K_SB, 4): return x.template step<Sb<4>>(n);
    case code(K_SB, 8): return x.template step<Sb<8>>(n);
    case code(K_SB, 16): return x.template step<Sb<16>>(n);
    case code(K_SB_TABLES, 4): return x.template step<SbTables<4>>(n);
    case code(K_SB_TABLES, 8): return x.template step<SbTables<8>>(n);
    case code(K_SB_TABLES, 16): return x.template step<SbTables<16>>(n);
#if defined(__HIPCC__)
    case code(K_KT_BASES_QUAD, 5): return x.template step<KtBasesQuad<5>>(n);
    case code(K_KT_BASES_QUAD, 6): return x.template step<KtBasesQuad<6>>(n);
    case code(K_SB_TABLES_QUAD, 4): return x.template step<SbTablesQuad<4>>(n);
    case code(K_SB_TABLES_QUAD, 8): return x.template step<SbTablesQuad<8>>(n);
    case code(K_SB_TABLES_QUAD, 16): return x.template step<SbTablesQuad<16>>(n);
#endif
    default: return 3;
    }
}
// Every record of `in` in turn; x.pos is the read position, x.out collects the outputs.  One failing record ends the run.
template <typename X>
int run_records(X& x) {
    while (x.pos < x.in_words) {
        if (x.in_words - x.pos < 2) return 1;
        const uint32_t c = x.in[x.pos], n = x.in[x.pos + 1];
        x.pos += 2;
        const int rc = dispatch(x, c, n);
        if (rc) return rc;
        ++x.records;
    }
    return 0;
}
// what an executor checks before it runs a record: the items are there and the buffers stay small
template <typename S>
bool record_fits(size_t in_words, size_t pos, uint32_t n) {
    return n != 0 && n <= (1u << 16) && (in_words - pos) / (size_t)S::IN >= n &&
           (size_t)n * ((size_t)S::OUT + (size_t)S::SCRATCH) <= ((size_t)1 << 28);
}

}  // namespace sc
}  // namespace jjs

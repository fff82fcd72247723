// What turns the two input formats into affine points, one stage per function, with caller-chosen inputs: the inversion by
// division steps (fq_inv.h: fq_inverse), the inverse square root with its byte-at-a-time logarithm and the point decoding
// built on it (decode.h: fq_inv_sqrt, decompress_point), the shared inversion of the extended-coordinate inputs
// (normalize.h: normalize_lane), and the square-root tables themselves.  ONE copy of the stage bodies and of the record
// format, compiled into tests/hostbuild/host_harness.cpp (CPU build) and tools/ingestcheck.hip (device): the two cannot
// drift.  The stages only execute; tests/ingest_cases.py writes the inputs and checks every output word with Python integers.
//
//   item records:   uint32 code, uint32 count, count * Stage::IN uint32          ->  count * Stage::OUT uint32
//   K_NORMALIZE:    uint32 code (kind << 24 | n_src), uint32 rows, uint32 n, first, lanes, 0,
//                   n_src arrays of rows x 24 uint32 (U | V | Z)
//                   ->  n_src arrays of rows x 16 uint32 (u | v), then norm_bad_words(rows) uint32 holding one byte per row.
//                       normalize_lane(P, lane, lanes) runs for every lane on the rows [first, first + n); the executor
//                       prefills the affine rows with NORM_FILL and the bytes with 0 inside the range, NORM_FILL_BYTE outside.
//   K_TABLES:       uint32 code, uint32 1  ->  the executor's own tables: DLOG_POW_WORDS uint32, then 65536 bytes as 16384 uint32
#pragma once
#include <vector>

#include "decode.h"
#include "fq_inv.h"
#include "normalize.h"

namespace jjs {
namespace ig {

// the test reads this enum
enum Kind : uint32_t { K_INV = 1, K_INV_SQRT, K_DECOMPRESS, K_NORMALIZE, K_TABLES, K_FINISH, K_UPDATE };
constexpr uint32_t code(uint32_t kind, uint32_t param = 0) { return kind << 24 | param; }

constexpr uint32_t NORM_FILL = 0xC3A55A3Cu, NORM_FILL_BYTE = 0xC3u;
constexpr uint32_t NORM_HEADER = 4, NORM_MAX_ROWS = 1u << 16, DLOG_HASH_BYTES = 65536;
constexpr size_t TABLES_OUT = (size_t)DLOG_POW_WORDS + DLOG_HASH_BYTES / 4;

struct ctx {
    dlog_tables T;        // built by the executor with dlog_table_entry after a cleared hash, as the library builds them
};

JJS_HD words8 ld8(const uint32_t* p) {
    words8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = p[i];
    return r;
}
JJS_HD void st8(uint32_t* o, const words8& w) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = w.w[i];
}

// a (8, canonical)  ->  1 / a (8), 0 for 0
struct Inv {
    static constexpr int IN = 8, OUT = 8;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out) { st8(out, fq_to_words(fq_inverse(fq_from_words(ld8(in))))); }
};
// d (9 signed limbs of 30 bits, value in (-2q, q)) | sign (1) | 0 (2)  ->  normalize_30(d, sign) (9) | 0 (1): the end of fq_inverse
// on its own, with the values of d that no input of fq_inverse leaves there (the idle batches after g = 0 lift d to [0, q))
struct Finish {
    static constexpr int IN = 12, OUT = 10;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out) {
        s30 d;
#pragma unroll
        for (int i = 0; i < 9; ++i) d.v[i] = (int32_t)in[i];
        normalize_30(d, (int32_t)in[9]);
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = (uint32_t)d.v[i];
        out[9] = 0u;
    }
};
// d (9) | e (9) | u, v, q, r (4) | 0 (2)  ->  d' (9) | e' (9) | 0 (2): update_de_30 on its own, with d and e over the whole of
// (-2q, q) in both sign combinations and with matrices at |u| + |v| = 2^30 -- the operands for which its sign terms exist, and
// which fq_inverse's own inputs do not come near
struct Update {
    static constexpr int IN = 24, OUT = 20;
    JJS_HD static void run(const ctx&, const uint32_t* in, uint32_t* out) {
        s30 d, e;
#pragma unroll
        for (int i = 0; i < 9; ++i) { d.v[i] = (int32_t)in[i]; e.v[i] = (int32_t)in[9 + i]; }
        divstep_matrix t;
        t.u = (int32_t)in[18]; t.v = (int32_t)in[19]; t.q = (int32_t)in[20]; t.r = (int32_t)in[21];
        update_de_30(d, e, t);
#pragma unroll
        for (int i = 0; i < 9; ++i) { out[i] = (uint32_t)d.v[i]; out[9 + i] = (uint32_t)e.v[i]; }
        out[18] = out[19] = 0u;
    }
};
// y (8, canonical)  ->  fq_inv_sqrt(y) (8): y^((t-1)/2) * zeta^(-(k >> 1)) with zeta^k = y^t, for squares and non-squares alike
struct InvSqrt {
    static constexpr int IN = 8, OUT = 8;
    JJS_HD static void run(const ctx& C, const uint32_t* in, uint32_t* out) { st8(out, fq_to_words(fq_inv_sqrt(fq_from_words(ld8(in)), C.T))); }
};
// 32 bytes (8)  ->  u (8) | v (8) | ok (1) | 0 (3)
struct Decompress {
    static constexpr int IN = 8, OUT = 20;
    JJS_HD static void run(const ctx& C, const uint32_t* in, uint32_t* out) {
        const decoded_point d = decompress_point(ld8(in), C.T);
        st8(out, d.u);
        st8(out + 8, d.v);
        out[16] = d.ok ? 1u : 0u;
        out[17] = out[18] = out[19] = 0u;
    }
};

// ---- K_NORMALIZE ----------------------------------------------------------------------------------------------------------
struct norm_header {
    uint32_t n_src, rows, n, first, lanes;
};
constexpr size_t norm_bad_words(uint32_t rows) { return ((size_t)rows + 3) / 4; }
constexpr size_t norm_in_words(uint32_t n_src, uint32_t rows) { return NORM_HEADER + (size_t)n_src * rows * 24; }
constexpr size_t norm_out_words(uint32_t n_src, uint32_t rows) { return (size_t)n_src * rows * 16 + norm_bad_words(rows); }
constexpr size_t norm_scratch_words(uint32_t rows) { return 9 * (size_t)rows + 4; }
// the header at `p` (NORM_HEADER words) is one that normalize_lane can run inside buffers of `rows` rows
inline bool norm_header_ok(uint32_t n_src, uint32_t rows, const uint32_t* p, norm_header& H) {
    H = norm_header{n_src, rows, p[0], p[1], p[2]};
    return n_src >= 1 && n_src <= 4 && rows >= 1 && rows <= NORM_MAX_ROWS && H.n >= 1 && H.n <= rows && H.first <= rows - H.n &&
           H.lanes >= 1 && H.lanes <= NORM_MAX_ROWS && p[3] == 0;
}
// `ext`: the n_src input arrays one after the other; `out`: the affine arrays one after the other, then the bytes
inline normalize_params norm_params(const norm_header& H, const uint32_t* ext, uint32_t* out, uint32_t* scratch) {
    normalize_params P{};
    P.n_src = H.n_src; P.n = H.n; P.first = H.first; P.scratch = scratch;
    for (uint32_t k = 0; k < H.n_src; ++k) {
        P.src[k] = fe_src{reinterpret_cast<const uint8_t*>(ext + (size_t)k * H.rows * 24), 96, 0};
        P.out[k] = reinterpret_cast<uint8_t*>(out + (size_t)k * H.rows * 16);
    }
    P.bad = reinterpret_cast<uint8_t*>(out + (size_t)H.n_src * H.rows * 16);
    return P;
}
// the output of a K_NORMALIZE record before any lane runs (host memory)
inline void norm_prefill(const norm_header& H, uint32_t* out) {
    const size_t aff = (size_t)H.n_src * H.rows * 16;
    for (size_t i = 0; i < aff; ++i) out[i] = NORM_FILL;
    uint8_t* bad = reinterpret_cast<uint8_t*>(out + aff);
    for (size_t i = 0; i < 4 * norm_bad_words(H.rows); ++i) bad[i] = (i >= H.first && i < (size_t)H.first + H.n) ? 0 : (uint8_t)NORM_FILL_BYTE;
}

// One record through executor X: step<Stage>(count) runs an item stage, normalize(n_src, rows) and tables(count) the other
// two.  Non-zero: unknown code or X's error.
template <typename X>
int dispatch(X& x, uint32_t c, uint32_t n) {
    switch (c) {
    case code(K_INV): return x.template step<Inv>(n);
    case code(K_INV_SQRT): return x.template step<InvSqrt>(n);
    case code(K_DECOMPRESS): return x.template step<Decompress>(n);
    case code(K_NORMALIZE, 1): case code(K_NORMALIZE, 2): case code(K_NORMALIZE, 3): case code(K_NORMALIZE, 4):
        return x.normalize(c & 0xffu, n);
    case code(K_FINISH): return x.template step<Finish>(n);
    case code(K_UPDATE): return x.template step<Update>(n);
    case code(K_TABLES): return x.tables(n);
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
// what an executor checks before it runs an item record: the items are there and the buffers stay small
template <typename S>
bool record_fits(size_t in_words, size_t pos, uint32_t n) {
    return n != 0 && n <= (1u << 16) && (in_words - pos) / (size_t)S::IN >= n;
}
inline bool norm_fits(size_t in_words, size_t pos, uint32_t n_src, uint32_t rows, const uint32_t* in, norm_header& H) {
    return in_words - pos >= NORM_HEADER && norm_header_ok(n_src, rows, in + pos, H) && in_words - pos >= norm_in_words(n_src, rows);
}

}  // namespace ig
}  // namespace jjs

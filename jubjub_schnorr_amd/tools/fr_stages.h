// The scalar arithmetic modulo the group order r and what produces and consumes its scalars, one stage per function, with
// caller-chosen inputs: fr_mont_mul, fr_mul, fr_sub_mul, fr_add and half_scalar_times_u (verify_core.h), truncate250
// (hades29.h), chacha20_block and bv_weights (batch_verdict.h).  ONE copy of the stage bodies and of the record format,
// compiled into tests/hostbuild/host_harness.cpp (CPU build) and tools/frcheck.hip (device, one lane per item, whole waves):
// the two cannot drift.  The stages only execute; tests/fr_cases.py writes the inputs and checks every output word with Python
// integers and a ChaCha20 written from RFC 8439.
//
//   records:  uint32 code, uint32 count, count * Stage::IN uint32      code = kind << 24
//   output:   per record, count * Stage::OUT uint32
#pragma once
#include <stddef.h>

#include "batch_verdict.h"
#include "hades29.h"

namespace jjs {
namespace fr {

// the test reads this enum
enum Kind : uint32_t { K_MONT_MUL = 1, K_MUL, K_SUB_MUL, K_ADD, K_HALF_TIMES_U, K_TRUNCATE250, K_CHACHA20, K_WEIGHTS };
constexpr uint32_t code(uint32_t kind) { return kind << 24; }

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

// a (8) | b (8)  ->  a b 2^-256 mod r (8)
struct MontMul {
    static constexpr int IN = 16, OUT = 8;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) { st8(out, fr_mont_mul(ld8(in), ld8(in + 8))); }
};
// a (8) | b (8)  ->  a b mod r (8)
struct Mul {
    static constexpr int IN = 16, OUT = 8;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) { st8(out, fr_mul(ld8(in), ld8(in + 8))); }
};
// a (8) | b (8) | c (8)  ->  a - b c mod r (8)
struct SubMul {
    static constexpr int IN = 24, OUT = 8;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) { st8(out, fr_sub_mul(ld8(in), ld8(in + 8), ld8(in + 16))); }
};
// a (8) | b (8)  ->  a + b mod r (8)
struct Add {
    static constexpr int IN = 16, OUT = 8;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) { st8(out, fr_add(ld8(in), ld8(in + 8))); }
};
// |b| (4) | sign of b (1) | pad (3) | u (8)  ->  b u mod r (8)
struct HalfTimesU {
    static constexpr int IN = 16, OUT = 8;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) {
        half_scalars h{};
        for (int i = 0; i < 4; ++i) h.b.w[i] = in[i];
        h.b_neg = in[4] != 0u;
        st8(out, half_scalar_times_u(h, ld8(in + 8)));
    }
};
// x (8, below q) | representative (1) | pad (3)  ->  truncate250 (8) | the limbs differ from fq_from_words(x)'s (1) | 0 (1)
// fe_n holds values below 2q, so a residue has two representatives: 0 is the one fq_from_words returns, 1 the other one
// (that one + q when it is below q, - q otherwise).
struct Truncate250 {
    static constexpr int IN = 12, OUT = 10;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) {
        const fe_n f = fq_from_words(ld8(in));
        fe_c q;
#pragma unroll
        for (int i = 0; i < 9; ++i) q.l[i] = q29(i);
        const fe_n other = fq_reduce(fq_norm(fq_add(f, q)));        // f + q below 3q; minus 2q when that reaches 2q
        const fe_n g = fq_select(in[8] != 0u, other, f);
        st8(out, truncate250(g));
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) diff |= g.l[i] ^ f.l[i];
        out[8] = diff != 0u ? 1u : 0u;
        out[9] = 0u;
    }
};
// key (8) | counter (1) | nonce (3)  ->  the block (16)
struct ChaCha20 {
    static constexpr int IN = 12, OUT = 16;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) {
        uint32_t key[8], nonce[3], b[16];
        for (int i = 0; i < 8; ++i) key[i] = in[i];
        for (int i = 0; i < 3; ++i) nonce[i] = in[9 + i];
        chacha20_block(key, in[8], nonce, b);
        for (int i = 0; i < 16; ++i) out[i] = b[i];
    }
};
// seed (8) | item, low and high word (2) | bits (1) | pad (1)  ->  z (8) | z' (8)
struct Weights {
    static constexpr int IN = 12, OUT = 16;
    JJS_HD static void run(const uint32_t* in, uint32_t* out) {
        uint32_t seed[8];
        for (int i = 0; i < 8; ++i) seed[i] = in[i];
        words8 z, zp;
        bv_weights(seed, (uint64_t)in[8] | (uint64_t)in[9] << 32, (int)in[10], z, zp);
        st8(out, z);
        st8(out + 8, zp);
    }
};

// One record through executor X, whose step<Stage>(count) runs the stage on every item.  Non-zero: unknown code or X's error.
template <typename X>
int dispatch(X& x, uint32_t c, uint32_t n) {
    switch (c) {
    case code(K_MONT_MUL): return x.template step<MontMul>(n);
    case code(K_MUL): return x.template step<Mul>(n);
    case code(K_SUB_MUL): return x.template step<SubMul>(n);
    case code(K_ADD): return x.template step<Add>(n);
    case code(K_HALF_TIMES_U): return x.template step<HalfTimesU>(n);
    case code(K_TRUNCATE250): return x.template step<Truncate250>(n);
    case code(K_CHACHA20): return x.template step<ChaCha20>(n);
    case code(K_WEIGHTS): return x.template step<Weights>(n);
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
    return n != 0 && n <= (1u << 20) && (in_words - pos) / (size_t)S::IN >= n;
}

}  // namespace fr
}  // namespace jjs

// Device-only arithmetic at the edges of its static bounds: the generated blocks (tools/gen_mont_asm.py) in every copy the
// device runs -- mont_mul_call / mont_mul_inl and the squares, fq_mul_hot, fq_mul_chain, fq_sqr_plus_const, the Hades linear
// layer -- the canonical form behind fq_to_words / fq_is_zero / fq_eq, the cooperative permutation (hades_permute, eight lanes)
// and the quad doubling (ext_double_quad, four lanes).  This program only executes: tests/test_device_edges_gpu.py writes the
// inputs, runs it once and checks every output limb against Python big integers.  Every bound class is its own template
// instantiation, so the static_asserts of fq29.h hold for what runs here.
//
//   edgecheck IN OUT
//   IN : records of  uint32 code, uint32 count, count * in_words(code) uint32
//        code = kind << 24 | La << 20 | Aa << 12 | Lb << 8 | Ab   (the bound class; 0 where unused)
//   OUT: per record, count * out_words(code) uint32
// One launch per record.  An unknown code, a short file or a HIP error ends it with a non-zero status.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "hades29.h"
#include "ed29_quad.h"

using namespace jjs;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// the test reads this enum and the class lists below
enum Kind { K_MUL_CALL = 1, K_MUL_INL, K_MUL_HOT, K_MUL_CHAIN, K_SQR_CALL, K_SQR_INL, K_SQR_HOT, K_SQR_PLUS_CONST, K_SQR_CHAIN,
            K_HADES_MATRIX, K_LINCOMB, K_TO_WORDS, K_IS_ZERO, K_EQ, K_PERMUTE, K_PERMUTE_COOP, K_DOUBLE, K_DOUBLE_QUAD, K_ADD_NIELS };

// (La, Aa, Lb, Ab)
#define MUL_HOT_CLASSES(X) X(1, 2, 1, 2) X(1, 70, 1, 1) X(1, 1, 1, 70) X(1, 7, 3, 10) X(3, 10, 1, 7) X(1, 35, 3, 2) X(3, 2, 1, 35) X(3, 8, 1, 8)
#define MUL_CHAIN_CLASSES(X) X(2, 2, 2, 2) X(2, 3, 2, 3) X(2, 35, 2, 2) X(2, 8, 2, 8) X(1, 70, 4, 1) X(4, 1, 1, 70) X(1, 5, 4, 14) X(4, 14, 1, 5) X(1, 2, 2, 3)
// (La, Aa)
#define SQR_HOT_CLASSES(X) X(1, 1) X(1, 2) X(1, 4) X(1, 8)
#define SQR_PLUS_CONST_CLASSES(X) X(2, 3)
#define SQR_CHAIN_CLASSES(X) X(1, 2) X(1, 8) X(2, 3)
#define TO_WORDS_CLASSES(X) X(1, 1) X(1, 2) X(1, 4) X(3, 5) X(1, 70) X(7, 9)
#define IS_ZERO_CLASSES(X) X(1, 2) X(3, 4) X(3, 5) X(5, 9) X(7, 70)
// (La, Aa, Ab): fq_eq(fe<La, Aa>, fe<1, Ab>)
#define EQ_CLASSES(X) X(1, 2, 1) X(1, 2, 2) X(3, 5, 3) X(5, 20, 4)

constexpr uint32_t code(uint32_t kind, uint32_t la = 0, uint32_t aa = 0, uint32_t lb = 0, uint32_t ab = 0) {
    return kind << 24 | la << 20 | aa << 12 | lb << 8 | ab;
}

template <int L, int A>
__device__ __forceinline__ fe<L, A> ld(const uint32_t* p) {
    fe<L, A> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = p[i];
    return r;
}
__device__ __forceinline__ void st(uint32_t* o, const uint32_t* l, int n = 9) {
    for (int i = 0; i < n; ++i) o[i] = l[i];
}
__device__ __forceinline__ ext_pt ld_pt(const uint32_t* p) {
    ext_pt r;
    r.x = ld<1, 2>(p); r.y = ld<1, 2>(p + 9); r.z = ld<1, 2>(p + 18); r.t = ld<1, 2>(p + 27);
    return r;
}
__device__ __forceinline__ void st_pt(uint32_t* o, const ext_pt& p) {
    st(o, p.x.l); st(o + 9, p.y.l); st(o + 18, p.z.l); st(o + 27, p.t.l);
}

// One functor per stage: LANES lanes per item (aligned groups), IN words in, OUT words out per item; j = lane in the group.
struct MulCall {
    static constexpr int LANES = 1, IN = 18, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        st(o, mont_mul_call(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11], x[12], x[13], x[14], x[15],
                            x[16], x[17]).l);
    }
};
struct MulInl {
    static constexpr int LANES = 1, IN = 18, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        st(o, mont_mul_inl(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11], x[12], x[13], x[14], x[15],
                           x[16], x[17]).l);
    }
};
template <int La, int Aa, int Lb, int Ab>
struct MulHot {
    static constexpr int LANES = 1, IN = 18, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st(o, fq_mul_hot(ld<La, Aa>(x), ld<Lb, Ab>(x + 9)).l); }
};
template <int La, int Aa, int Lb, int Ab>
struct MulChain {
    static constexpr int LANES = 1, IN = 18, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st(o, fq_mul_chain(ld<La, Aa>(x), ld<Lb, Ab>(x + 9)).l); }
};
struct SqrCall {
    static constexpr int LANES = 1, IN = 9, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        st(o, mont_sqr_call(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8]).l);
    }
};
struct SqrInl {
    static constexpr int LANES = 1, IN = 9, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        st(o, mont_sqr_inl(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8]).l);
    }
};
template <int La, int Aa>
struct SqrHot {
    static constexpr int LANES = 1, IN = 9, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st(o, fq_sqr_hot(ld<La, Aa>(x)).l); }
};
template <int La, int Aa>
struct SqrPlusConst {
    static_assert(La == 2, "fq_sqr_plus_const takes fe<2, A>");
    static constexpr int LANES = 1, IN = 9, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st(o, fq_sqr_plus_const(ld<2, Aa>(x)).l); }
};
template <int La, int Aa>
struct SqrChain {
    static constexpr int LANES = 1, IN = 9, OUT = 9;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st(o, fq_sqr_chain(ld<La, Aa>(x)).l); }
};
struct HadesMatrix {
    static constexpr int LANES = 1, IN = 45, OUT = 45;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        fe_n t[5];
        for (int j = 0; j < 5; ++j) t[j] = ld<1, 2>(x + 9 * j);
        hades_state s;
        hades_matrix(s, t);
        for (int i = 0; i < 5; ++i) st(o + 9 * i, s.s[i].l);
    }
};
struct Lincomb {    // the rows of the cooperative hash: S[i][k] = JJS_HS_HANKEL[i + k]
    static constexpr int LANES = 1, IN = 45, OUT = 45;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        fe_n t[5];
        for (int j = 0; j < 5; ++j) t[j] = ld<1, 2>(x + 9 * j);
        for (int i = 0; i < 5; ++i) st(o + 9 * i, fq_lincomb_small<5>(JJS_HS_HANKEL + i, t).l);
    }
};
template <int L, int A>
struct ToWords {
    static constexpr int LANES = 1, IN = 9, OUT = 8;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st(o, fq_to_words(ld<L, A>(x)).w, 8); }
};
template <int L, int A>
struct IsZero {
    static constexpr int LANES = 1, IN = 9, OUT = 1;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { o[0] = fq_is_zero(ld<L, A>(x)) ? 1u : 0u; }
};
template <int La, int Aa, int Ab>
struct Eq {
    static constexpr int LANES = 1, IN = 18, OUT = 1;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { o[0] = fq_eq(ld<La, Aa>(x), ld<1, Ab>(x + 9)) ? 1u : 0u; }
};
struct Permute {
    static constexpr int LANES = 1, IN = 45, OUT = 45;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        hades_state s;
        for (int i = 0; i < 5; ++i) s.s[i] = ld<1, 2>(x + 9 * i);
        hades_permute(s);
        for (int i = 0; i < 5; ++i) st(o + 9 * i, s.s[i].l);
    }
};
struct PermuteCoop {   // every lane of the eight writes the state it ends with
    static constexpr int LANES = 8, IN = 45, OUT = 8 * 45;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t j) const {
        hades_state s;
        for (int i = 0; i < 5; ++i) s.s[i] = ld<1, 2>(x + 9 * i);
        hades_permute(s, (int)j);
        for (int i = 0; i < 5; ++i) st(o + 45 * j + 9 * i, s.s[i].l);
    }
};
struct Double {
    static constexpr int LANES = 1, IN = 36, OUT = 36;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const { st_pt(o, ext_double(ld_pt(x), true)); }
};
struct DoubleQuad {    // every lane of the four writes 2P and its own product (coordinate j of 2P)
    static constexpr int LANES = 4, IN = 36, OUT = 4 * 45;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t j) const {
        fe_n own;
        const ext_pt r = ext_double_quad(ld_pt(x), j, own);
        st_pt(o + 45 * j, r);
        st(o + 45 * j + 36, own.l);
    }
};
struct AddNiels {      // P (36 words) + the cached addend (ypx, ymx, z, t2d: fe<1, 5> each) with neg = word 72
    static constexpr int LANES = 1, IN = 73, OUT = 36;
    __device__ void operator()(const uint32_t* x, uint32_t* o, uint32_t) const {
        niels_pt n;
        n.ypx = ld<1, 5>(x + 36); n.ymx = ld<1, 5>(x + 45); n.z = ld<1, 5>(x + 54); n.t2d = ld<1, 5>(x + 63);
        st_pt(o, ext_add_niels(ld_pt(x), n, x[72] != 0, true));
    }
};

template <typename F>
__global__ void __launch_bounds__(64) k_run(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x, item = t / F::LANES, j = t % F::LANES;
    if (item < n) F()(in + (size_t)F::IN * item, out + (size_t)F::OUT * item, j);    // whole groups leave together
}

template <typename F>
static int step(const std::vector<uint32_t>& in, size_t& pos, uint32_t n, std::vector<uint32_t>& out) {
    const size_t in_words = (size_t)F::IN * n, out_words = (size_t)F::OUT * n;
    if (n == 0 || n > (1u << 20) || in.size() - pos < in_words) {
        fprintf(stderr, "record of %u items does not fit the input\n", n);
        return 1;
    }
    uint32_t *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, in_words * 4));
    CHECK(hipMalloc(&dout, out_words * 4));
    CHECK(hipMemcpy(din, in.data() + pos, in_words * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(dout, 0xff, out_words * 4));
    const uint32_t threads = n * F::LANES;
    hipLaunchKernelGGL(k_run<F>, dim3((threads + 63) / 64), dim3(64), 0, 0, din, dout, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    const size_t at = out.size();
    out.resize(at + out_words);
    CHECK(hipMemcpy(out.data() + at, dout, out_words * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    pos += in_words;
    return 0;
}

static int dispatch(uint32_t c, const std::vector<uint32_t>& in, size_t& pos, uint32_t n, std::vector<uint32_t>& out) {
#define MUL_HOT_CASE(la, aa, lb, ab) case code(K_MUL_HOT, la, aa, lb, ab): return step<MulHot<la, aa, lb, ab>>(in, pos, n, out);
#define MUL_CHAIN_CASE(la, aa, lb, ab) case code(K_MUL_CHAIN, la, aa, lb, ab): return step<MulChain<la, aa, lb, ab>>(in, pos, n, out);
#define SQR_HOT_CASE(la, aa) case code(K_SQR_HOT, la, aa): return step<SqrHot<la, aa>>(in, pos, n, out);
#define SQR_PLUS_CONST_CASE(la, aa) case code(K_SQR_PLUS_CONST, la, aa): return step<SqrPlusConst<la, aa>>(in, pos, n, out);
#define SQR_CHAIN_CASE(la, aa) case code(K_SQR_CHAIN, la, aa): return step<SqrChain<la, aa>>(in, pos, n, out);
#define TO_WORDS_CASE(l, a) case code(K_TO_WORDS, l, a): return step<ToWords<l, a>>(in, pos, n, out);
#define IS_ZERO_CASE(l, a) case code(K_IS_ZERO, l, a): return step<IsZero<l, a>>(in, pos, n, out);
#define EQ_CASE(la, aa, ab) case code(K_EQ, la, aa, 1, ab): return step<Eq<la, aa, ab>>(in, pos, n, out);
    switch (c) {
    case code(K_MUL_CALL): return step<MulCall>(in, pos, n, out);
    case code(K_MUL_INL): return step<MulInl>(in, pos, n, out);
    MUL_HOT_CLASSES(MUL_HOT_CASE)
    MUL_CHAIN_CLASSES(MUL_CHAIN_CASE)
    case code(K_SQR_CALL): return step<SqrCall>(in, pos, n, out);
    case code(K_SQR_INL): return step<SqrInl>(in, pos, n, out);
    SQR_HOT_CLASSES(SQR_HOT_CASE)
    SQR_PLUS_CONST_CLASSES(SQR_PLUS_CONST_CASE)
    SQR_CHAIN_CLASSES(SQR_CHAIN_CASE)
    case code(K_HADES_MATRIX): return step<HadesMatrix>(in, pos, n, out);
    case code(K_LINCOMB): return step<Lincomb>(in, pos, n, out);
    TO_WORDS_CLASSES(TO_WORDS_CASE)
    IS_ZERO_CLASSES(IS_ZERO_CASE)
    EQ_CLASSES(EQ_CASE)
    case code(K_PERMUTE): return step<Permute>(in, pos, n, out);
    case code(K_PERMUTE_COOP): return step<PermuteCoop>(in, pos, n, out);
    case code(K_DOUBLE): return step<Double>(in, pos, n, out);
    case code(K_DOUBLE_QUAD): return step<DoubleQuad>(in, pos, n, out);
    case code(K_ADD_NIELS): return step<AddNiels>(in, pos, n, out);
    default:
        fprintf(stderr, "unknown stage code %08x\n", c);
        return 3;
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: edgecheck IN OUT\n");
        return 1;
    }
    std::vector<uint32_t> in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        uint32_t buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
        fclose(f);
    }
    std::vector<uint32_t> out;
    size_t pos = 0;
    int records = 0;
    while (pos < in.size()) {
        if (in.size() - pos < 2) { fprintf(stderr, "truncated record header\n"); return 1; }
        const uint32_t c = in[pos], n = in[pos + 1];
        pos += 2;
        const int rc = dispatch(c, in, pos, n, out);
        if (rc) return rc;
        ++records;
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(out.data(), 4, out.size(), g) != out.size() || fclose(g) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    printf("edgecheck: %d records, %zu output words\n", records, out.size());
    return 0;
}

// `is_valid` of the C++ header (include/jjs_schnorr.hpp: is_valid() on the six types, jjs::is_valid_batch).
// Built with -DJJS_STUB it links no engine: the two host calls are defined here, record what the header marshalled and answer with
// statuses chosen from the first byte of every item, so that the columns, their widths and the mapping to bool are checked on
// any machine.  Built without, it links libjjs_gpu.so and checks a few known points on the GPU.  Exit code 0 = all met.
#include <cstdio>

#include "jjs_schnorr.hpp"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

#if defined(JJS_STUB)
struct Recorded {
    int scheme = -1, format = -1;
    size_t n = 0;
    std::vector<uint8_t> col[3];
    bool has[3] = {}, wants[3] = {};
} last;
static const uint8_t kStatus[4] = {0, 1, 3, 0};
static void record(Recorded& r, int i, const uint8_t* p, size_t bytes) {
    r.has[i] = p != nullptr;
    r.col[i].assign(p ? p : (const uint8_t*)"", p ? p + bytes : (const uint8_t*)"");
}
extern "C" {
const char* jjs_last_error(void) { return "stub"; }
int jjs_keys_check(int scheme, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint8_t* status, uint64_t tally[4], uint8_t* A0_out,
                   uint8_t* A1_out) {
    if (scheme == 77) return JJS_ERR_ARG;
    last = Recorded{};
    last.scheme = scheme; last.format = format; last.n = n;
    const size_t two = scheme == JJS_SCHEME_SINGLE ? 1 : 2;
    const size_t w = format == JJS_FORMAT_WIRE ? 32 * two : (format == JJS_FORMAT_EXT ? 96 : 64);
    record(last, 0, K0, n * w); record(last, 1, K1, n * w);
    last.wants[0] = A0_out != nullptr; last.wants[1] = A1_out != nullptr;
    for (size_t i = 0; i < n; ++i) status[i] = kStatus[K0[i * w] & 3];
    if (A0_out) for (size_t i = 0; i < n * 64; ++i) A0_out[i] = (uint8_t)(i * 7);
    (void)tally;
    return JJS_OK;
}
int jjs_signatures_check(int scheme, int format, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, size_t n, uint8_t* status, uint64_t tally[4],
                         uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out) {
    last = Recorded{};
    last.scheme = scheme; last.format = format; last.n = n;
    record(last, 0, s0, n * 32); record(last, 1, s1, n * 64); record(last, 2, s2, n * 64);
    last.wants[0] = u_out != nullptr; last.wants[1] = R_out != nullptr; last.wants[2] = Rp_out != nullptr;
    for (size_t i = 0; i < n; ++i) status[i] = kStatus[s0[i * 32] & 3];
    (void)tally;
    return JJS_OK;
}
}

template <size_t N>
static std::array<uint8_t, N> filled(uint8_t first, uint8_t rest) {
    std::array<uint8_t, N> a;
    a.fill(rest);
    a[0] = first;
    return a;
}
template <size_t N>
static bool holds(const std::vector<uint8_t>& col, size_t i, const std::array<uint8_t, N>& v) {
    return col.size() >= (i + 1) * N && std::memcmp(col.data() + i * N, v.data(), N) == 0;
}

int main() {
    const size_t n = 5;
    const bool want[5] = {true, false, false, true, true};           // first bytes 0, 1, 2, 3, 4 -> statuses 0, 1, 3, 0, 0
    std::vector<jjs::PublicKey> ks; std::vector<jjs::PublicKeyDouble> kd; std::vector<jjs::PublicKeyVarGen> kv;
    std::vector<jjs::Signature> ss; std::vector<jjs::SignatureDouble> sd; std::vector<jjs::SignatureVarGen> sv;
    std::vector<jjs::ExtendedPoint> ke; std::vector<jjs::PointBytes> kb;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t b = (uint8_t)i;
        ks.emplace_back(filled<64>(b, 0x10));
        kd.emplace_back(filled<64>(b, 0x20), filled<64>(9, 0x21));
        kv.emplace_back(filled<64>(b, 0x30), filled<64>(9, 0x31));
        ss.push_back({filled<32>(b, 0x40), filled<64>(9, 0x41)});
        sd.push_back({filled<32>(b, 0x50), filled<64>(9, 0x51), filled<64>(8, 0x52)});
        sv.push_back({filled<32>(b, 0x60), filled<64>(9, 0x61)});
        ke.push_back(filled<96>(b, 0x70));
        kb.push_back(filled<32>(b, 0x80));
    }
    auto same = [&](const std::vector<bool>& got) { bool ok = got.size() == n; for (size_t i = 0; ok && i < n; ++i) ok = got[i] == want[i]; return ok; };

    EXPECT(same(jjs::is_valid_batch(ks)));
    EXPECT(last.scheme == JJS_SCHEME_SINGLE && last.format == JJS_FORMAT_AFFINE && last.n == n && last.has[0] && !last.has[1] && !last.wants[0] && !last.wants[1]);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, ks[i].as_ref()));
    EXPECT(same(jjs::is_valid_batch(kd)));
    EXPECT(last.scheme == JJS_SCHEME_DOUBLE && last.format == JJS_FORMAT_AFFINE && last.has[0] && last.has[1]);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, kd[i].pk()) && holds(last.col[1], i, kd[i].pk_prime()));
    EXPECT(same(jjs::is_valid_batch(kv)));
    EXPECT(last.scheme == JJS_SCHEME_VARGEN && last.format == JJS_FORMAT_AFFINE);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, kv[i].public_key()) && holds(last.col[1], i, kv[i].generator()));

    EXPECT(same(jjs::is_valid_batch(ss)));
    EXPECT(last.scheme == JJS_SCHEME_SINGLE && last.format == JJS_FORMAT_AFFINE && last.has[0] && last.has[1] && !last.has[2]);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, ss[i].u) && holds(last.col[1], i, ss[i].R));
    EXPECT(same(jjs::is_valid_batch(sd)));
    EXPECT(last.scheme == JJS_SCHEME_DOUBLE && last.has[2] && !last.wants[0] && !last.wants[1] && !last.wants[2]);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, sd[i].u) && holds(last.col[1], i, sd[i].R) && holds(last.col[2], i, sd[i].R_prime));
    EXPECT(same(jjs::is_valid_batch(sv)));
    EXPECT(last.scheme == JJS_SCHEME_VARGEN && !last.has[2]);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, sv[i].u) && holds(last.col[1], i, sv[i].R));

    std::vector<jjs::AffinePoint> affine;
    EXPECT(same(jjs::is_valid_batch(ke)));
    EXPECT(last.scheme == JJS_SCHEME_SINGLE && last.format == JJS_FORMAT_EXT && !last.has[1] && !last.wants[0]);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, ke[i]));
    EXPECT(same(jjs::is_valid_batch(kb, &affine)));
    EXPECT(last.format == JJS_FORMAT_WIRE && last.wants[0] && !last.wants[1] && affine.size() == n);
    for (size_t i = 0; i < n; ++i) EXPECT(holds(last.col[0], i, kb[i]));
    for (size_t i = 0; i < affine.size(); ++i) for (size_t j = 0; j < 64; ++j) EXPECT(affine[i][j] == (uint8_t)((64 * i + j) * 7));

    for (size_t i = 0; i < n; ++i) {
        EXPECT(ks[i].is_valid() == want[i] && kd[i].is_valid() == want[i] && kv[i].is_valid() == want[i]);
        EXPECT(last.n == 1);
        EXPECT(ss[i].is_valid() == want[i] && sd[i].is_valid() == want[i] && sv[i].is_valid() == want[i]);
    }
    EXPECT(jjs::is_valid_batch(std::vector<jjs::PublicKey>{}).empty() && last.n == 0);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
#else
int main() {
    jjs::Engine engine;
    jjs::AffinePoint g{}, ident{}, big{};
    // the generator: u = 0x3fd2814c43ac65a6f1fbf02d0fd6cce62e3ebb21fd6c54ed4df7b7ffec7beaca, v = 0x12 (little-endian bytes)
    const uint8_t gu[32] = {0xca, 0xea, 0x7b, 0xec, 0xff, 0xb7, 0xf7, 0x4d, 0xed, 0x54, 0x6c, 0xfd, 0x21, 0xbb, 0x3e, 0x2e,
                            0xe6, 0xcc, 0xd6, 0x0f, 0x2d, 0xf0, 0xfb, 0xf1, 0xa6, 0x65, 0xac, 0x43, 0x4c, 0x81, 0xd2, 0x3f};
    std::memcpy(g.data(), gu, 32); g[32] = 0x12;
    ident[32] = 1;
    big.fill(0xFF);
    jjs::JubJubScalar u{}, u_big;
    u[0] = 5; u_big.fill(0xFF);
    const std::vector<bool> k = jjs::is_valid_batch(std::vector<jjs::PublicKey>{jjs::PublicKey(g), jjs::PublicKey(ident), jjs::PublicKey(big)});
    EXPECT(k.size() == 3 && k[0] && !k[1] && !k[2]);
    EXPECT(jjs::PublicKey(g).is_valid() && !jjs::PublicKey(ident).is_valid());
    EXPECT(jjs::PublicKeyDouble(g, g).is_valid() && !jjs::PublicKeyDouble(g, ident).is_valid() && !jjs::PublicKeyVarGen(ident, g).is_valid());
    EXPECT((jjs::Signature{u, g}.is_valid()) && !(jjs::Signature{u_big, g}.is_valid()) && !(jjs::SignatureVarGen{u, ident}.is_valid()));
    EXPECT((jjs::SignatureDouble{u, g, g}.is_valid()) && !(jjs::SignatureDouble{u, g, big}.is_valid()));
    jjs::ExtendedPoint e{};
    std::memcpy(e.data(), g.data(), 64); e[64] = 1;                  // Z = 1
    jjs::PointBytes w{};
    w[0] = 0x12; w[31] = (uint8_t)((gu[0] & 1) << 7);               // v, the parity of u in bit 255
    std::vector<jjs::AffinePoint> a, b;
    EXPECT(jjs::is_valid_batch(std::vector<jjs::ExtendedPoint>{e}, &a)[0] && a.size() == 1 && a[0] == g);
    EXPECT(jjs::is_valid_batch(std::vector<jjs::PointBytes>{w}, &b)[0] && b.size() == 1 && b[0] == g);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
#endif

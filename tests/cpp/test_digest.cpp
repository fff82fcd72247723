// jjs::poseidon::digest, digest_truncated and digest_batch of the C++ header (include/jjs_schnorr.hpp).
// Built with -DJJS_STUB it links no engine: jjs_digest is defined here, records what the header marshalled and answers with rows
// derived from the input, so that the column, the offsets, the flag and the mapping of statuses are checked on any machine.  Built
// without, it links libjjs_gpu.so and checks the reference's single challenge on the GPU.  Exit code 0 = all met.
#include <cstdio>

#include "jjs_schnorr.hpp"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static jjs::BlsScalar scalar(uint8_t first, uint8_t rest = 0) {
    jjs::BlsScalar s;
    s.fill(rest);
    s[0] = first;
    return s;
}

#if defined(JJS_STUB)
struct Recorded {
    int format = -1, flags = -1;
    size_t k = 99, n = 0;
    std::vector<uint32_t> offsets;
    std::vector<uint8_t> in;
    bool has_status = false;
} last;
extern "C" {
const char* jjs_last_error(void) { return "stub"; }
// status 3 for an item whose first byte is 0xEE; row i = (first byte of the item, its length, the flags, 0...)
int jjs_digest(int format, int flags, const uint8_t* in, const uint32_t* offsets, size_t k, size_t n, uint8_t* out, uint8_t* status) {
    if (n && offsets && offsets[1] == offsets[0]) return JJS_ERR_ARG;
    last = Recorded{};
    last.format = format; last.flags = flags; last.k = k; last.n = n; last.has_status = status != nullptr;
    last.offsets.assign(offsets, offsets + n + 1);
    last.in.assign(in, in + 32 * (size_t)offsets[n]);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t first = in[32 * (size_t)offsets[i]];
        status[i] = first == 0xEE ? 3 : 0;
        for (int b = 0; b < 32; ++b) out[32 * i + b] = 0;
        if (status[i]) continue;
        out[32 * i] = first; out[32 * i + 1] = (uint8_t)(offsets[i + 1] - offsets[i]); out[32 * i + 2] = (uint8_t)flags;
    }
    return JJS_OK;
}
}

int main() {
    using namespace jjs;
    const std::vector<std::vector<BlsScalar>> payloads = {{scalar(1), scalar(2), scalar(3)}, {scalar(0xEE)}, {scalar(7, 9), scalar(8)}};
    const auto d = poseidon::digest_batch(payloads);
    EXPECT(last.format == JJS_DIGEST_CANONICAL && last.flags == 0 && last.n == 3 && last.k == 0 && last.has_status);
    EXPECT((last.offsets == std::vector<uint32_t>{0, 3, 4, 6}));
    EXPECT(last.in.size() == 6 * 32 && last.in[0] == 1 && last.in[32] == 2 && last.in[96] == 0xEE && last.in[128] == 7 && last.in[129] == 9 &&
           last.in[160] == 8);
    EXPECT(d.size() == 3 && d[0] && !d[1] && d[2]);
    EXPECT((*d[0])[0] == 1 && (*d[0])[1] == 3 && (*d[0])[2] == 0 && (*d[2])[0] == 7 && (*d[2])[1] == 2);
    const auto t = poseidon::digest_batch(payloads, true);
    EXPECT(last.flags == JJS_DIGEST_TRUNCATED && t[0] && (*t[0])[2] == JJS_DIGEST_TRUNCATED);
    const auto one = poseidon::digest({scalar(5), scalar(6)});
    EXPECT(last.n == 1 && last.flags == 0 && one && (*one)[0] == 5 && (*one)[1] == 2);
    const auto cut = poseidon::digest_truncated({scalar(5)});
    EXPECT(last.n == 1 && last.flags == JJS_DIGEST_TRUNCATED && cut && (*cut)[1] == 1);
    EXPECT(!poseidon::digest({scalar(0xEE)}));
    EXPECT(poseidon::digest_batch({}).empty() && last.n == 0);
    bool threw = false;
    try { poseidon::digest({}); } catch (const EngineError& e) { threw = e.code == JJS_ERR_ARG; }
    EXPECT(threw);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
#else
int main() {
    using namespace jjs;
    Engine engine;
    // digest_truncated of (1, 2, 3, 4, 5) twice gives one value, the low 250 bits of digest; a scalar >= q is refused
    const std::vector<BlsScalar> payload = {scalar(1), scalar(2), scalar(3), scalar(4), scalar(5)};
    const auto full = poseidon::digest(payload);
    const auto cut = poseidon::digest_truncated(payload);
    EXPECT(full && cut);
    if (full && cut) {
        BlsScalar masked = *full;
        masked[31] &= 0x03;
        EXPECT(masked == *cut);
        EXPECT(*full != scalar(0));
    }
    const auto batch = poseidon::digest_batch({payload, {scalar(0xFF, 0xFF)}, {scalar(9)}});
    EXPECT(batch.size() == 3 && batch[0] && *batch[0] == *full && !batch[1] && batch[2]);
    bool threw = false;
    try { poseidon::digest({}); } catch (const EngineError& e) { threw = e.code == JJS_ERR_ARG; }
    EXPECT(threw);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
#endif

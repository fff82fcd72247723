// jjs::KeySet (include/jjs_schnorr.hpp) the way a validator-set client uses it: the keys registered once, then
// (index, signature, message) batches; the expected statuses come from the golden vectors, as in test_schnorr.cpp.
// Inputs: a text file, one vector per line: scheme name expected_status hex-fields (the argument order of the inline call).
// Exit code 0 = all expectations met.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "jjs_schnorr.hpp"

template <size_t N>
static std::array<uint8_t, N> unhex(const std::string& s) {
    std::array<uint8_t, N> out{};
    if (s.size() != 2 * N) throw std::runtime_error("bad hex length");
    for (size_t i = 0; i < N; ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}
static int code(const jjs::VerifyResult& r) {
    return !r ? 0 : (*r == jjs::Error::InvalidPoint ? 1 : (*r == jjs::Error::InvalidSignature ? 2 : 3));
}

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_keyset vectors.txt"); return 2; }
    jjs::Engine engine;
    std::ifstream in(argv[1]);
    std::string line;
    std::vector<jjs::PublicKey> ks; std::vector<jjs::KeySet::Item<jjs::Signature>> is; std::vector<int> ws;
    std::vector<jjs::PublicKeyDouble> kd; std::vector<jjs::KeySet::Item<jjs::SignatureDouble>> id; std::vector<int> wd;
    std::vector<jjs::PublicKeyVarGen> kv; std::vector<jjs::KeySet::Item<jjs::SignatureVarGen>> iv; std::vector<int> wv;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string scheme, name, a, b, c, d, e, g;
        int want = 0;
        f >> scheme >> name >> want;
        if (scheme == "single") {
            f >> a >> b >> c >> d;
            ks.emplace_back(unhex<64>(c));
            is.push_back({(uint32_t)(ks.size() - 1), jjs::Signature{unhex<32>(a), unhex<64>(b)}, unhex<32>(d)});
            ws.push_back(want);
        } else if (scheme == "double") {
            f >> a >> b >> c >> d >> e >> g;
            kd.emplace_back(unhex<64>(d), unhex<64>(e));
            id.push_back({(uint32_t)(kd.size() - 1), jjs::SignatureDouble{unhex<32>(a), unhex<64>(b), unhex<64>(c)}, unhex<32>(g)});
            wd.push_back(want);
        } else if (scheme == "vargen") {
            f >> a >> b >> c >> d >> e;
            kv.emplace_back(unhex<64>(c), unhex<64>(d));
            iv.push_back({(uint32_t)(kv.size() - 1), jjs::SignatureVarGen{unhex<32>(a), unhex<64>(b)}, unhex<32>(e)});
            wv.push_back(want);
        }
    }
    int failures = 0, total = 0;
    auto check = [&](const std::vector<jjs::VerifyResult>& got, const std::vector<int>& want, const char* what) {
        for (size_t i = 0; i < got.size(); ++i, ++total)
            if (code(got[i]) != want[i]) { std::printf("FAIL %s %zu: got %d want %d\n", what, i, code(got[i]), want[i]); ++failures; }
    };
    jjs::KeySet a(ks), b(kd), c(kv);
    check(a.verify_batch(is), ws, "single");
    check(b.verify_batch(id), wd, "double");
    jjs::KeySet moved(std::move(c));                 // move-only: the handle travels, the source is empty
    check(moved.verify_batch(iv), wv, "vargen");
    if (c.handle() != 0 || moved.info()[JJS_KEYSET_KEYS] != kv.size()) { std::puts("FAIL move"); ++failures; }
    std::printf("%d vectors, %d failures\n", total, failures);
    return failures ? 1 : 0;
}

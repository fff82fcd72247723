// jjs::KeySet::add / reserve / growth (include/jjs_schnorr.hpp) the way a validator-set client uses them across epochs: half
// the keys registered, the other half added -- once appended behind a reserve, once offered again as unique candidates -- then
// (index, signature, message) batches against old and new indices; the expected statuses come from the golden vectors.
// Input: a text file, one single-scheme vector per line: name expected_status u R PK m (hex).  Exit code 0 = all met.
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
    if (argc < 2) { std::puts("usage: test_keyset_add vectors.txt"); return 2; }
    jjs::Engine engine;
    std::ifstream in(argv[1]);
    std::string line;
    std::vector<jjs::PublicKey> keys;
    std::vector<jjs::KeySet::Item<jjs::Signature>> items;
    std::vector<int> want;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string name, u, r, pk, m;
        int st = 0;
        f >> name >> st >> u >> r >> pk >> m;
        keys.emplace_back(unhex<64>(pk));
        items.push_back({(uint32_t)(keys.size() - 1), jjs::Signature{unhex<32>(u), unhex<64>(r)}, unhex<32>(m)});
        want.push_back(st);
    }
    const size_t n = keys.size(), half = n / 2;
    if (half == 0) { std::puts("too few vectors"); return 2; }
    int failures = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++failures; } };
    jjs::KeySet ks(std::vector<jjs::PublicKey>(keys.begin(), keys.begin() + half));
    ks.reserve(n);
    expect(ks.growth()[JJS_KEYSET_CAPACITY] == n && ks.growth()[JJS_KEYSET_RELOCATIONS] == 1, "reserve");
    const jjs::KeySet::Added a = ks.add(std::vector<jjs::PublicKey>(keys.begin() + half, keys.end()));
    expect(a.n_added == n - half && a.idx.size() == n - half, "n_added");
    for (size_t i = 0; i < a.idx.size(); ++i) expect(a.idx[i] == half + i, "appended index");
    expect(ks.info()[JJS_KEYSET_KEYS] == n && ks.key_status().size() == n, "keys");
    expect(ks.growth()[JJS_KEYSET_RELOCATIONS] == 1 && ks.growth()[JJS_KEYSET_ADD_CALLS] == 1, "an add that fits moves nothing");
    const std::vector<jjs::VerifyResult> got = ks.verify_batch(items);
    for (size_t i = 0; i < n; ++i)
        if (code(got[i]) != want[i]) { std::printf("FAIL item %zu: got %d want %d\n", i, code(got[i]), want[i]); ++failures; }
    // every key offered again, unique: nothing is registered, and each is answered with the index jjs_keyset_find gives
    const std::vector<uint32_t> found = ks.find(keys);
    const jjs::KeySet::Added again = ks.add(keys, true);
    expect(again.n_added == 0 && ks.info()[JJS_KEYSET_KEYS] == n, "unique: nothing new");
    for (size_t i = 0; i < n; ++i) expect(again.idx[i] == found[i] && (found[i] == 0xFFFFFFFFu) == (again.key_status[i] == 3), "unique index");
    std::printf("%zu vectors, %d failures\n", n, failures);
    return failures ? 1 : 0;
}

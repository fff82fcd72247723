// jjs::KeySet::remove / compact / removal (include/jjs_schnorr.hpp) the way a validator-set client uses them when validators
// rotate out: every key registered, every second one removed -- the items that name them fail at once, the others verify as
// before, at their old indices -- then the set compacted and the surviving items verified at the indices the map gives; the
// expected statuses come from the golden vectors.
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
    if (argc < 2) { std::puts("usage: test_keyset_remove vectors.txt"); return 2; }
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
    const size_t n = keys.size();
    if (n < 2) { std::puts("too few vectors"); return 2; }
    int failures = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++failures; } };
    jjs::KeySet ks(keys);
    const std::vector<uint8_t> registered = ks.key_status();
    std::vector<uint32_t> odd;
    for (size_t i = 1; i < n; i += 2) odd.push_back((uint32_t)i);
    odd.push_back((uint32_t)n);                       // beyond the set
    odd.push_back(1);                                 // named twice
    const jjs::KeySet::Removed r = ks.remove(odd);
    expect(r.n_removed == n / 2 && r.result.size() == odd.size(), "n_removed");
    for (size_t k = 0; k + 2 < odd.size(); ++k) expect(r.result[k] == registered[odd[k]], "the status before the remove");
    expect(r.result[odd.size() - 2] == JJS_KEY_NOT_IN_RANGE && r.result.back() == registered[1], "out of range / named twice");
    expect(ks.info()[JJS_KEYSET_KEYS] == n && ks.removal()[JJS_KEYSET_REMOVED_KEYS] == n / 2 && ks.removal()[JJS_KEYSET_LIVE_KEYS] == n - n / 2, "counts");
    std::vector<jjs::VerifyResult> got = ks.verify_batch(items);
    for (size_t i = 0; i < n; ++i) {
        const int w = i % 2 ? 3 : want[i];
        if (code(got[i]) != w) { std::printf("FAIL item %zu after the remove: got %d want %d\n", i, code(got[i]), w); ++failures; }
        expect(ks.key_status()[i] == (i % 2 ? 3 : registered[i]), "key_status follows");
    }
    expect(ks.remove(odd).n_removed == 0, "removing again removes nothing");
    const std::vector<uint32_t> map = ks.compact();
    expect(map.size() == n && ks.info()[JJS_KEYSET_KEYS] == n - n / 2 && ks.key_status().size() == n - n / 2, "compacted");
    expect(ks.removal()[JJS_KEYSET_REMOVED_KEYS] == 0 && ks.removal()[JJS_KEYSET_COMPACT_CALLS] == 1 && ks.growth()[JJS_KEYSET_RELOCATIONS] == 1, "counters");
    std::vector<jjs::KeySet::Item<jjs::Signature>> kept;
    std::vector<int> kept_want;
    for (size_t i = 0; i < n; ++i) {
        expect(map[i] == (i % 2 ? 0xFFFFFFFFu : (uint32_t)(i / 2)), "the map");
        if (i % 2) continue;
        kept.push_back({map[i], items[i].sig, items[i].message});
        kept_want.push_back(want[i]);
    }
    got = ks.verify_batch(kept);
    for (size_t i = 0; i < kept.size(); ++i)
        if (code(got[i]) != kept_want[i]) { std::printf("FAIL item %zu after the compact: got %d want %d\n", i, code(got[i]), kept_want[i]); ++failures; }
    std::printf("%zu vectors, %d failures\n", n, failures);
    return failures ? 1 : 0;
}

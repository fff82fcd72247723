// jjs::KeySet::multisig_combine (include/jjs_schnorr.hpp) the way a validator set's client uses it: the keys registered once,
// then one transcript of an ordered subset, named by index.  Input: a text file of hex lines -- "keys" (n_keys x 64 bytes),
// "status" (n_keys), "idx" (n x 4, little-endian), "z" (n x 32), "R", "S" (n x 96 extended), "m" (32), then the expected "u" (32)
// and "rsa" (64), and "bad" (4): the index of an unusable key.  The program checks the good transcript, the same with share 1
// spoilt (InvalidMultisigShare(1)) and the same with row 2 naming the unusable key (BytesError(2)).  Exit code 0 = all met.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

#include "jjs_schnorr.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}
template <typename Row>
static std::vector<Row> rows(const std::vector<uint8_t>& bytes) {
    std::vector<Row> out(bytes.size() / sizeof(Row));
    for (size_t i = 0; i < out.size(); ++i) std::memcpy(out[i].data(), bytes.data() + sizeof(Row) * i, sizeof(Row));
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_msig_keyset transcript.txt"); return 2; }
    std::map<std::string, std::vector<uint8_t>> f;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string key, hex;
        ls >> key >> hex;
        f[key] = unhex(hex);
    }
    jjs::Engine engine;
    const size_t n_keys = f["keys"].size() / 64, n = f["z"].size() / 32;
    jjs::KeySet set(JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, f["keys"].data(), nullptr, n_keys);
    int failures = 0;
    if (set.key_status() != f["status"]) { std::puts("FAIL key_status"); ++failures; }
    std::vector<uint32_t> idx(n);
    std::memcpy(idx.data(), f["idx"].data(), 4 * n);
    uint32_t bad = 0;
    std::memcpy(&bad, f["bad"].data(), 4);
    const auto z = rows<jjs::JubJubScalar>(f["z"]);
    const auto R = rows<jjs::ExtendedPoint>(f["R"]), S = rows<jjs::ExtendedPoint>(f["S"]);
    jjs::BlsScalar m;
    std::memcpy(m.data(), f["m"].data(), 32);

    const auto good = set.multisig_combine(idx, z, R, S, m);
    if (!good || good.error) { std::puts("FAIL the good transcript gives no signature"); ++failures; }
    else if (std::memcmp(good.signature->u.data(), f["u"].data(), 32) != 0 || std::memcmp(good.signature->R.data(), f["rsa"].data(), 64) != 0) {
        std::puts("FAIL signature"); ++failures;
    }
    auto z_bad = z;
    z_bad[1][0] ^= 1;
    const auto spoilt = set.multisig_combine(idx, z_bad, R, S, m);
    if (spoilt || !spoilt.error || spoilt.error->kind != jjs::multisig::CombineError::InvalidMultisigShare || spoilt.error->participant_index != 1) {
        std::puts("FAIL a spoilt share is InvalidMultisigShare(1)"); ++failures;
    }
    auto idx_bad = idx;
    idx_bad[2] = bad;
    const auto refused = set.multisig_combine(idx_bad, z, R, S, m);
    if (refused || !refused.error || refused.error->kind != jjs::multisig::CombineError::BytesError || refused.error->participant_index != 2) {
        std::puts("FAIL a refused transcript is BytesError(2)"); ++failures;
    }
    idx_bad[2] = (uint32_t)n_keys;
    const auto outside = set.multisig_combine(idx_bad, z, R, S, m);
    if (outside || !outside.error || outside.error->kind != jjs::multisig::CombineError::BytesError || outside.error->participant_index != 2) {
        std::puts("FAIL an index outside the set is BytesError(2)"); ++failures;
    }
    const auto empty = set.multisig_combine({}, {}, {}, {}, m);
    if (empty || empty.error->kind != jjs::multisig::CombineError::InvalidMultisigTranscript) { std::puts("FAIL empty transcript"); ++failures; }
    std::printf("%zu keys, %zu participants, %d failures\n", n_keys, n, failures);
    return failures ? 1 : 0;
}

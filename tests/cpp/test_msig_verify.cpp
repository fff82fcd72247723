// jjs::multisig::aggregate_pk / verify and jjs::KeySet::multisig_aggregate_pk / multisig_verify (include/jjs_schnorr.hpp) the
// way a verifier uses them: a key vector, a message and an aggregate signature.  Input: a text file of hex lines -- "keys"
// (n_keys x 64 bytes), "idx" (n x 4, little-endian), "pk" (n x 96 extended: the same keys), "u" (32), "R" (64), "m" (32), the
// expected "agg" (64), and "bad" (4): the index of an unusable key.  The program checks the good vector, the same with u
// spoilt (InvalidSignature) and the same with key 2 unusable (Z = 0 inline, the bad index for the set: refused, BytesError),
// in the single and the batch form, and the empty vector (the identity; InvalidPoint).  Exit code 0 = all met.
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
static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAIL %s\n", what); ++failures; }
}
static bool is(const jjs::VerifyResult& r, jjs::Error e) { return r.has_value() && *r == e; }

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_msig_verify vector.txt"); return 2; }
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
    const size_t n_keys = f["keys"].size() / 64, n = f["pk"].size() / 96;
    jjs::KeySet set(JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, f["keys"].data(), nullptr, n_keys);
    std::vector<uint32_t> idx(n);
    std::memcpy(idx.data(), f["idx"].data(), 4 * n);
    uint32_t bad = 0;
    std::memcpy(&bad, f["bad"].data(), 4);
    const auto pk = rows<jjs::ExtendedPoint>(f["pk"]);
    jjs::Signature sig;
    jjs::BlsScalar m;
    jjs::AffinePoint want, identity{}, zero{};
    identity[32] = 1;
    std::memcpy(sig.u.data(), f["u"].data(), 32);
    std::memcpy(sig.R.data(), f["R"].data(), 64);
    std::memcpy(m.data(), f["m"].data(), 32);
    std::memcpy(want.data(), f["agg"].data(), 64);

    // inline keys
    const auto agg = jjs::multisig::aggregate_pk(pk);
    expect(agg && *agg == want, "aggregate_pk");
    jjs::AffinePoint got{};
    expect(!jjs::multisig::verify(pk, sig, m, &got) && got == want, "the good vector verifies");
    jjs::Signature spoilt = sig;
    spoilt.u[0] ^= 1;
    expect(is(jjs::multisig::verify(pk, spoilt, m), jjs::Error::InvalidSignature), "a spoilt u is InvalidSignature");
    auto pk_bad = pk;
    std::memset(pk_bad[2].data() + 64, 0, 32);                   // Z = 0
    expect(!jjs::multisig::aggregate_pk(pk_bad), "a vector with an unusable key has no aggregate");
    expect(is(jjs::multisig::verify(pk_bad, sig, m, &got), jjs::Error::BytesError) && got == zero, "a refused vector is BytesError");
    const auto none = jjs::multisig::aggregate_pk({});
    expect(none && *none == identity, "the empty vector aggregates to the identity");
    expect(is(jjs::multisig::verify({}, sig, m), jjs::Error::InvalidPoint), "the empty vector is InvalidPoint");
    uint64_t tally[4] = {9, 9, 9, 9};
    std::vector<jjs::AffinePoint> aggs;
    const auto batch = jjs::multisig::verify_batch({{pk, sig, m}, {pk, spoilt, m}, {pk_bad, sig, m}, {{}, sig, m}}, &aggs, tally);
    expect(batch.size() == 4 && !batch[0] && is(batch[1], jjs::Error::InvalidSignature) && is(batch[2], jjs::Error::BytesError) &&
               is(batch[3], jjs::Error::InvalidPoint), "the batch form");
    expect(aggs.size() == 4 && aggs[0] == want && aggs[1] == want && aggs[2] == zero && aggs[3] == identity, "the batch form's aggregates");
    expect(tally[0] == 1 && tally[1] == 1 && tally[2] == 1 && tally[3] == 1, "the batch form's tally");

    // the same keys named by index into the set
    const auto kagg = set.multisig_aggregate_pk(idx);
    expect(kagg && *kagg == want, "KeySet::multisig_aggregate_pk");
    expect(!set.multisig_verify(idx, sig, m, &got) && got == want, "KeySet: the good vector verifies");
    expect(is(set.multisig_verify(idx, spoilt, m), jjs::Error::InvalidSignature), "KeySet: a spoilt u is InvalidSignature");
    auto idx_bad = idx;
    idx_bad[2] = bad;
    expect(!set.multisig_aggregate_pk(idx_bad), "KeySet: a vector naming an unusable key has no aggregate");
    expect(is(set.multisig_verify(idx_bad, sig, m, &got), jjs::Error::BytesError) && got == zero, "KeySet: a refused vector is BytesError");
    idx_bad[2] = (uint32_t)n_keys;
    expect(is(set.multisig_verify(idx_bad, sig, m), jjs::Error::BytesError), "KeySet: an index outside the set is BytesError");
    std::printf("%zu keys, %zu in the vector, %d failures\n", n_keys, n, failures);
    return failures ? 1 : 0;
}

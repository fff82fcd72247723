// The overloads of jjs::multisig (include/jjs_schnorr.hpp) that take `to_bytes` forms, the way a shim that receives the data from
// the network uses them: one transcript of compressed points through jjs_multisig_combine_wire, the verifier's half from
// PublicKey::to_bytes and Signature::to_bytes, and a SignerGroup registered from the same wire keys.  Input: a text file of hex
// lines -- "pk", "R", "S" (n x 32 bytes each), "z" (n x 32), "m" (32), "sig" (64 = u || R, the expected signature), then the
// expected affine "agg" (64) and "rsa" (64), "bad" (32: an encoding that does not decode) and "spoil" (one byte: the participant
// whose z the program spoils).  Exit code 0 = all expectations met.
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
template <class T>
static std::vector<T> rows(const std::vector<uint8_t>& flat) {
    std::vector<T> out(flat.size() / sizeof(T));
    for (size_t i = 0; i < out.size(); ++i) std::memcpy(out[i].data(), flat.data() + sizeof(T) * i, sizeof(T));
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_msig_wire transcript.txt"); return 2; }
    std::map<std::string, std::vector<uint8_t>> f;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string key, hex;
        ls >> key >> hex;
        f[key] = unhex(hex);
    }
    using namespace jjs;
    using multisig::CombineError;
    Engine engine;
    auto pk = rows<PointBytes>(f["pk"]), R = rows<PointBytes>(f["R"]), S = rows<PointBytes>(f["S"]);
    auto z = rows<JubJubScalar>(f["z"]);
    BlsScalar m;
    std::memcpy(m.data(), f["m"].data(), 32);
    SignatureBytes sig;
    std::memcpy(sig.data(), f["sig"].data(), 64);
    PointBytes bad_point;
    std::memcpy(bad_point.data(), f["bad"].data(), 32);
    int failures = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++failures; } };

    // the combiner
    const auto good = multisig::combine(z, pk, R, S, m);
    expect(bool(good) && !good.error, "the transcript combines");
    if (good) {
        expect(std::memcmp(good.signature->u.data(), sig.data(), 32) == 0, "u");
        expect(std::memcmp(good.signature->R.data(), f["rsa"].data(), 64) == 0, "R");
    }
    const size_t spoil = f["spoil"][0];
    auto z_bad = z;
    z_bad[spoil][0] ^= 1;
    const auto bad = multisig::combine(z_bad, pk, R, S, m);
    expect(!bad && bad.error && bad.error->kind == CombineError::InvalidMultisigShare && bad.error->participant_index == spoil, "index of the spoilt share");
    auto R_bad = R;
    R_bad[0] = bad_point;                                                // what from_bytes rejects
    z_bad[spoil] = z[spoil];
    z_bad.back()[0] ^= 1;
    const auto first = multisig::combine(z_bad, pk, R_bad, S, m);
    expect(!first && first.error && first.error->kind == CombineError::BytesError && first.error->participant_index == 0, "the FIRST failing share");
    const auto empty = multisig::combine({}, {}, {}, {}, m);             // (the extended form: braces deduce no wire overload)
    expect(!empty && empty.error && empty.error->kind == CombineError::InvalidMultisigTranscript, "empty transcript");
    const auto empty_w = multisig::combine({}, std::vector<PointBytes>{}, std::vector<PointBytes>{}, std::vector<PointBytes>{}, m);
    expect(!empty_w && empty_w.error && empty_w.error->kind == CombineError::InvalidMultisigTranscript, "empty wire transcript");

    // the verifier
    const auto agg = multisig::aggregate_pk(pk);
    expect(agg && std::memcmp(agg->data(), f["agg"].data(), 64) == 0, "aggregate_pk from wire keys");
    auto pk_bad = pk;
    pk_bad[1] = bad_point;
    expect(!multisig::aggregate_pk(pk_bad), "a vector with an undecodable key has no aggregate");
    AffinePoint a{};
    expect(!multisig::verify(pk, sig, m, &a) && std::memcmp(a.data(), f["agg"].data(), 64) == 0, "the aggregate signature verifies");
    SignatureBytes flipped = sig;
    flipped[0] ^= 1;
    const auto wrong = multisig::verify(pk, flipped, m);
    expect(wrong && *wrong == Error::InvalidSignature, "one bit of u flipped");
    SignatureBytes no_r = sig;
    std::memcpy(no_r.data() + 32, bad_point.data(), 32);
    uint64_t tally[4] = {9, 9, 9, 9};
    const auto batch = multisig::verify_batch(std::vector<multisig::VerifyItemBytes>{{pk, sig, m}, {pk, no_r, m}, {pk_bad, sig, m}}, nullptr, tally);
    expect(batch.size() == 3 && !batch[0] && batch[1] && *batch[1] == Error::BytesError && batch[2] && *batch[2] == Error::BytesError, "the batch form");
    expect(tally[0] == 1 && tally[3] == 2 && tally[0] + tally[1] + tally[2] + tally[3] == 3, "the tally sums to the items");

    // the group
    multisig::SignerGroup group(pk);
    expect(std::memcmp(group.aggregate_pk().data(), f["agg"].data(), 64) == 0, "aggregate_pk of the group from wire keys");
    const size_t n = pk.size();
    std::vector<uint8_t> st(n), ts(1), su(32), sr(64);
    group.combine_wire(f["z"].data(), f["R"].data(), f["S"].data(), f["m"].data(), 1, st.data(), ts.data(), su.data(), sr.data());
    expect(ts[0] == 0 && std::memcmp(su.data(), sig.data(), 32) == 0 && sr == f["rsa"], "the group's host call");
    bool refused = false;
    try { multisig::SignerGroup g2(pk_bad); } catch (const EngineError&) { refused = true; }
    expect(refused, "a group with an undecodable key is refused");
    std::printf("%zu participants, %d failures\n", n, failures);
    return failures ? 1 : 0;
}

// jjs::multisig::combine (include/jjs_schnorr.hpp) the way a shim for the Rust types uses it: one transcript of extended points
// through the blocking host form, and a SignerGroup registered from the same extended keys.  Input: a text file of hex lines --
// "pk", "R", "S" (n x 96 bytes each), "z" (n x 32), "m" (32), then the expected "agg" (64), "u" (32), "rsa" (64) and "spoil"
// (one byte: the participant whose z the program spoils).  Exit code 0 = all expectations met.
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
    if (argc < 2) { std::puts("usage: test_msig_ext transcript.txt"); return 2; }
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
    auto pk = rows<ExtendedPoint>(f["pk"]), R = rows<ExtendedPoint>(f["R"]), S = rows<ExtendedPoint>(f["S"]);
    auto z = rows<JubJubScalar>(f["z"]);
    BlsScalar m;
    std::memcpy(m.data(), f["m"].data(), 32);
    int failures = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++failures; } };

    const auto good = multisig::combine(z, pk, R, S, m);
    expect(bool(good) && !good.error, "the transcript combines");
    if (good) {
        expect(std::memcmp(good.signature->u.data(), f["u"].data(), 32) == 0, "u");
        expect(std::memcmp(good.signature->R.data(), f["rsa"].data(), 64) == 0, "R");
    }
    const size_t spoil = f["spoil"][0];
    auto z_bad = z;
    z_bad[spoil][0] ^= 1;
    const auto bad = multisig::combine(z_bad, pk, R, S, m);
    expect(!bad && bad.error && bad.error->kind == CombineError::InvalidMultisigShare && bad.error->participant_index == spoil, "index of the spoilt share");
    auto R_bad = R;
    std::memset(R_bad[0].data() + 64, 0, 32);                            // Z = 0: a value the Rust type cannot hold
    z_bad[spoil] = z[spoil];
    z_bad.back()[0] ^= 1;
    const auto first = multisig::combine(z_bad, pk, R_bad, S, m);
    expect(!first && first.error && first.error->kind == CombineError::BytesError && first.error->participant_index == 0, "the FIRST failing share");
    const auto empty = multisig::combine({}, {}, {}, {}, m);
    expect(!empty && empty.error && empty.error->kind == CombineError::InvalidMultisigTranscript, "empty transcript");
    auto z_short = z;
    z_short.pop_back();
    const auto uneven = multisig::combine(z_short, pk, R, S, m);
    expect(!uneven && uneven.error && uneven.error->kind == CombineError::InvalidMultisigTranscript, "vectors of unequal length");

    multisig::SignerGroup group(pk);
    expect(std::memcmp(group.aggregate_pk().data(), f["agg"].data(), 64) == 0, "aggregate_pk of the group from extended keys");
    const size_t n = pk.size();
    std::vector<uint8_t> st(n), ts(1), su(32), sr(64);
    group.combine(JJS_FORMAT_EXT, f["z"].data(), f["R"].data(), f["S"].data(), f["m"].data(), 1, st.data(), ts.data(), su.data(), sr.data());
    expect(ts[0] == 0 && su == f["u"] && sr == f["rsa"], "the group's host call");
    std::printf("%zu participants, %d failures\n", n, failures);
    return failures ? 1 : 0;
}

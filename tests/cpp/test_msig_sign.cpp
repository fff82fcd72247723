// jjs::multisig::sign_round_1 / sign_round_2 and CombineResult::first_failing_slot (include/jjs_schnorr.hpp) the way a signer uses
// them.  Input: a text file of hex lines for ONE transcript of n participants -- "sk", "r", "s" (n x 32), "pk", "R", "S" (n x 96
// extended, Z != 1), "Ra", "Sa" (n x 64: the affine nonce commitments), "m" (32) and the expected shares "z" (n x 32).
// Without a second argument only what needs no engine runs: sign_round_1 and the refusals of the host-side row search.  With
// "gpu": every signer's share, the row search in a permuted vector, the two new errors, BytesError, and the failing slot of
// `combine`.  Exit code 0 = all met.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <algorithm>
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
static bool is(const jjs::multisig::SignResult& r, jjs::Error e) { return !r.share && r.error && *r.error == e; }

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_msig_sign vector.txt [gpu]"); return 2; }
    const bool gpu = argc > 2 && std::string(argv[2]) == "gpu";
    std::map<std::string, std::vector<uint8_t>> f;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string key, hex;
        ls >> key >> hex;
        f[key] = unhex(hex);
    }
    namespace ms = jjs::multisig;
    const auto sk = rows<jjs::Scalar>(f["sk"]), r = rows<jjs::Scalar>(f["r"]), s = rows<jjs::Scalar>(f["s"]), z = rows<jjs::Scalar>(f["z"]);
    const auto pk = rows<jjs::ExtendedPoint>(f["pk"]), R = rows<jjs::ExtendedPoint>(f["R"]), S = rows<jjs::ExtendedPoint>(f["S"]);
    const auto Ra = rows<jjs::AffinePoint>(f["Ra"]), Sa = rows<jjs::AffinePoint>(f["Sa"]);
    jjs::BlsScalar m;
    std::memcpy(m.data(), f["m"].data(), 32);
    const size_t n = sk.size();

    // ---- no engine ----
    for (size_t i = 0; i < n; ++i) {
        const auto rs = ms::sign_round_1(r[i], s[i]);
        expect(rs.first == Ra[i] && rs.second == Sa[i], "sign_round_1 gives the fixture's R and S");
        expect(ms::host::same_point(R[i], Ra[i]) && !ms::host::same_point(R[i], Sa[i]), "the projective comparison of the row search");
    }
    jjs::Scalar other = sk[0];
    other[0] ^= 1;
    expect(is(ms::sign_round_2(other, r[0], s[0], pk, R, S, m), jjs::Error::InvalidMultisigTranscript), "a key that is not in pk_vec: refused without a call");
    auto twice = pk;
    twice[2] = twice[0];
    expect(is(ms::sign_round_2(sk[0], r[0], s[0], twice, R, S, m), jjs::Error::InvalidMultisigTranscript), "the signer's key twice: refused without a call");
    auto shorter = R;
    shorter.pop_back();
    expect(is(ms::sign_round_2(sk[0], r[0], s[0], pk, shorter, S, m), jjs::Error::InvalidMultisigTranscript), "vectors of unequal length: refused without a call");
    expect(is(ms::sign_round_2(sk[0], r[0], s[0], {}, {}, {}, m), jjs::Error::InvalidMultisigTranscript), "an empty transcript: refused without a call");
    ms::CombineResult none{std::nullopt, ms::CombineError{ms::CombineError::InvalidMultisigTranscript, 0}};
    ms::CombineResult slot{std::nullopt, ms::CombineError{ms::CombineError::InvalidMultisigShare, 2}};
    expect(!none.first_failing_slot() && slot.first_failing_slot() && *slot.first_failing_slot() == 2, "first_failing_slot of hand-made results");
    expect((int)jjs::Error::InvalidSignature == 0 && (int)jjs::Error::InvalidPoint == 1 && (int)jjs::Error::BytesError == 2 && (int)jjs::Error::Engine == 3,
           "the existing enumerators keep their values");

    if (gpu) {
        jjs::Engine engine;
        for (size_t i = 0; i < n; ++i) {
            const auto got = ms::sign_round_2(sk[i], r[i], s[i], pk, R, S, m);
            expect(got && *got.share == z[i], "sign_round_2 gives the expected share");
        }
        // the search finds the row wherever it is: rotate the three vectors by one
        auto rot = [&](auto v) { std::rotate(v.begin(), v.begin() + 1, v.end()); return v; };
        const auto moved = ms::sign_round_2(sk[0], r[0], s[0], rot(pk), rot(R), rot(S), m);
        expect(moved && *moved.share != z[0], "the signer found at the last row of a rotated transcript (another transcript: another share)");
        auto dupR = R;
        dupR[2] = dupR[1];
        expect(is(ms::sign_round_2(sk[0], r[0], s[0], pk, dupR, S, m), jjs::Error::DuplicatedNonce), "R twice among the others: DuplicatedNonce");
        expect(is(ms::sign_round_2(sk[0], r[1], s[0], pk, R, S, m), jjs::Error::InvalidMultisigTranscript), "r does not open R[i]: InvalidMultisigTranscript");
        auto badS = S;
        std::memset(badS[1].data() + 64, 0, 32);                    // Z = 0
        expect(is(ms::sign_round_2(sk[0], r[0], s[0], pk, R, badS, m), jjs::Error::BytesError), "an unusable point elsewhere: BytesError");
        const auto sig = ms::combine(z, pk, R, S, m);
        expect(bool(sig) && !sig.first_failing_slot(), "the shares combine");
        auto spoilt = z;
        spoilt[n - 1][0] ^= 1;
        const auto bad = ms::combine(spoilt, pk, R, S, m);
        expect(!bad && bad.error->kind == ms::CombineError::InvalidMultisigShare && bad.first_failing_slot() && *bad.first_failing_slot() == n - 1,
               "first_failing_slot names the spoilt share");
    }
    std::printf("%zu participants, %s, %d failures\n", n, gpu ? "with the engine" : "host only", failures);
    return failures ? 1 : 0;
}

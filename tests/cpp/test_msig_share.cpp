// jjs::multisig::verify_share, verify_share_batch, SignerGroup::verify_share and KeySet::multisig_verify_share
// (include/jjs_schnorr.hpp) the way a coordinator uses them.  Input: a text file of hex lines for ONE transcript of n participants --
// "pk", "R", "S" (n x 96 extended, Z != 1), "pkw", "Rw", "Sw" (n x 32: the to_bytes forms), "pka" (n x 64 affine), "m" (32), the
// shares "z" (n x 32) and the expected aggregate commitment "rsa" (64).
// Without a second argument only what needs no engine runs: the refusals decided on the host.  With "gpu": every share verifies, a
// wrong share is InvalidMultisigShare with ITS index, an out-of-range share BytesError, sig_R is the expected commitment, through
// every mirror.  Exit code 0 = all met.
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
namespace ms = jjs::multisig;
static bool is(const ms::ShareResult& r, ms::CombineError::Kind kind, size_t index) {
    return r && r->kind == kind && r->participant_index == index;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_msig_share vector.txt [gpu]"); return 2; }
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
    const auto z = rows<jjs::Scalar>(f["z"]);
    const auto pk = rows<jjs::ExtendedPoint>(f["pk"]), R = rows<jjs::ExtendedPoint>(f["R"]), S = rows<jjs::ExtendedPoint>(f["S"]);
    const auto pkw = rows<jjs::PointBytes>(f["pkw"]), Rw = rows<jjs::PointBytes>(f["Rw"]), Sw = rows<jjs::PointBytes>(f["Sw"]);
    const auto pka = rows<jjs::AffinePoint>(f["pka"]);
    jjs::BlsScalar m;
    std::memcpy(m.data(), f["m"].data(), 32);
    jjs::AffinePoint rsa;
    std::memcpy(rsa.data(), f["rsa"].data(), 64);
    const size_t n = pk.size();
    const auto T = ms::CombineError::InvalidMultisigTranscript;

    // ---- no engine: these answers are made on the host, as the reference makes them before any arithmetic ----
    expect(is(ms::verify_share(z[0], n, pk, R, S, m), T, 0), "participant_index == len: InvalidMultisigTranscript without a call");
    expect(is(ms::verify_share(z[0], n, pkw, Rw, Sw, m), T, 0), "... from bytes");
    auto shorter = R;
    shorter.pop_back();
    expect(is(ms::verify_share(z[0], 0, pk, shorter, S, m), T, 0), "vectors of unequal length: refused without a call");
    expect(is(ms::verify_share(z[0], 0, std::vector<jjs::ExtendedPoint>{}, std::vector<jjs::ExtendedPoint>{}, std::vector<jjs::ExtendedPoint>{}, m), T, 0),
           "an empty transcript: refused without a call");
    expect(ms::verify_share_batch({}, {}).empty(), "an empty batch");
    {
        const auto got = ms::verify_share_batch({}, {ms::ShareQuery{0, 0, z[0]}});
        expect(got.size() == 1 && is(got[0], T, 0), "a query without transcripts: refused without a call");
    }

    if (gpu) {
        jjs::Engine engine;
        const auto I = ms::CombineError::InvalidMultisigShare;
        for (size_t i = 0; i < n; ++i) {
            jjs::AffinePoint got_R{};
            expect(!ms::verify_share(z[i], i, pk, R, S, m, &got_R) && got_R == rsa, "verify_share ok, sig_R the aggregate commitment");
            expect(!ms::verify_share(z[i], i, pkw, Rw, Sw, m, &got_R) && got_R == rsa, "verify_share ok from bytes");
            expect(is(ms::verify_share(z[i], (i + 1) % n, pk, R, S, m), I, (i + 1) % n), "another signer's share: InvalidMultisigShare(index)");
        }
        jjs::Scalar wrong = z[1];
        wrong[0] ^= 1;
        expect(is(ms::verify_share(wrong, 1, pk, R, S, m), I, 1), "a wrong share: InvalidMultisigShare(1)");
        expect(is(ms::verify_share(wrong, 1, pkw, Rw, Sw, m), I, 1), "... from bytes");
        jjs::Scalar big;
        big.fill(0xFF);
        expect(is(ms::verify_share(big, 2, pk, R, S, m), ms::CombineError::BytesError, 2), "share >= r: BytesError(2)");
        auto bad_w = Rw;
        bad_w[0].fill(0xFF);
        expect(is(ms::verify_share(z[1], 1, pkw, bad_w, Sw, m), ms::CombineError::BytesError, 1), "an undecodable R: BytesError for every share");
        // the batch: two transcripts (the second of unequal vectors), queries in any order
        std::vector<jjs::AffinePoint> sig_R;
        const auto got = ms::verify_share_batch({ms::ShareTranscript{pk, R, S, m}, ms::ShareTranscript{pk, shorter, S, m}},
                                                {ms::ShareQuery{0, 2, z[2]}, ms::ShareQuery{1, 0, z[0]}, ms::ShareQuery{0, 0, wrong}, ms::ShareQuery{0, n, z[0]},
                                                 ms::ShareQuery{2, 0, z[0]}, ms::ShareQuery{0, 0, z[0]}},
                                                &sig_R);
        expect(got.size() == 6 && !got[0] && is(got[1], T, 0) && is(got[2], I, 0) && is(got[3], T, 0) && is(got[4], T, 0) && !got[5], "verify_share_batch");
        expect(sig_R.size() == 2 && sig_R[0] == rsa && sig_R[1] == jjs::AffinePoint{}, "verify_share_batch: sig_R");
        // a signer group and a key set
        ms::SignerGroup group(pk);
        jjs::AffinePoint got_R{};
        expect(!group.verify_share(z[0], 0, R, S, m, &got_R) && got_R == rsa, "SignerGroup::verify_share ok");
        expect(is(group.verify_share(wrong, 1, R, S, m), I, 1), "SignerGroup::verify_share: InvalidMultisigShare(1)");
        expect(is(group.verify_share(z[0], n, R, S, m), T, 0), "SignerGroup::verify_share: index == len");
        expect(group.info()[JJS_MSIG_GROUP_CALLS] == 2, "the group counted its two calls");
        jjs::KeySet set(JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, pka[0].data(), nullptr, n);
        std::vector<uint32_t> idx(n);
        for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)(n - 1 - i);           // the committee in reverse order of the set
        expect(is(set.multisig_verify_share(z[0], 0, idx, R, S, m), I, 0), "KeySet: the keys in another order are another transcript");
        for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
        expect(!set.multisig_verify_share(z[2], 2, idx, R, S, m, &got_R) && got_R == rsa, "KeySet::multisig_verify_share ok");
        expect(is(set.multisig_verify_share(wrong, 1, idx, R, S, m), I, 1), "KeySet::multisig_verify_share: InvalidMultisigShare(1)");
        idx[0] = 77;
        expect(is(set.multisig_verify_share(z[2], 2, idx, R, S, m), ms::CombineError::BytesError, 2), "KeySet: an index outside the set: BytesError");
    }
    std::printf("%zu participants, %s, %d failures\n", n, gpu ? "with the engine" : "host only", failures);
    return failures ? 1 : 0;
}

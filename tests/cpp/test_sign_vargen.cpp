// jjs::SecretKeyVarGen (include/jjs_schnorr.hpp) on the reference's own bytes.  Input: a text file of hex lines -- "secret" (64:
// serde_secret_key_var_gen = sk || generator compressed), "public" (64: pk || generator compressed), "signature" (64: u || R
// compressed), "m" and "rnd" (32 each: the message and the nonce's RNG draw behind the signature), "gen" (64: the generator affine).
// Without a second argument only what needs no engine runs: from_bytes / to_bytes and the compression of `new`'s generator.  With
// "gpu": public_key, sign and sign_batch against the bytes, the affine and the wire key alike, and one malformed key.
// Exit code 0 = all met.
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>

#include "jjs_schnorr.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}
template <size_t N>
static std::array<uint8_t, N> arr(const std::vector<uint8_t>& v, size_t at = 0) {
    std::array<uint8_t, N> a{};
    std::memcpy(a.data(), v.data() + at, N);
    return a;
}
static jjs::PointBytes compress(const jjs::AffinePoint& p) {
    jjs::PointBytes b = arr<32>(std::vector<uint8_t>(p.begin() + 32, p.end()));
    b[31] |= (uint8_t)((p[0] & 1) << 7);
    return b;
}
static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAIL %s\n", what); ++failures; }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_sign_vargen vector.txt [gpu]"); return 2; }
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
    const auto secret = arr<64>(f["secret"]), pub = arr<64>(f["public"]), signature = arr<64>(f["signature"]);
    const jjs::Scalar sk = arr<32>(f["secret"]), m = arr<32>(f["m"]), rnd = arr<32>(f["rnd"]);
    const jjs::AffinePoint gen = arr<64>(f["gen"]);

    // ---- no engine ----
    const jjs::SecretKeyVarGen wire = jjs::SecretKeyVarGen::from_bytes(secret);
    const jjs::SecretKeyVarGen affine = jjs::with_variable_generator(sk, gen);
    expect(wire.to_bytes() == secret, "from_bytes / to_bytes round trip");
    expect(affine.to_bytes() == secret, "new(sk, generator).to_bytes() compresses the generator");
    expect(wire.secret() == sk && jjs::SecretKeyVarGen(sk, gen).to_bytes() == secret, "the constructor is `new`");

    if (gpu) {
        jjs::Engine engine;
        for (const jjs::SecretKeyVarGen* k : {&wire, &affine}) {
            const auto pk = k->public_key();
            expect(pk && pk->generator() == gen, "public_key: the canonical affine generator");
            expect(pk && compress(pk->public_key()) == arr<32>(f["public"]) && compress(pk->generator()) == arr<32>(f["public"], 32),
                   "public_key gives serde_public_key_var_gen");
            const auto sig = k->sign(rnd, m);
            expect(sig && sig->u == arr<32>(f["signature"]) && compress(sig->R) == arr<32>(f["signature"], 32), "sign gives serde_signature_var_gen");
            expect(sig && pk && !pk->verify(*sig, m), "the signature verifies under the derived key");
        }
        auto bad_bytes = secret;
        std::memset(bad_bytes.data() + 32, 0xFF, 32);                     // v >= q: does not decode
        const jjs::SecretKeyVarGen bad = jjs::SecretKeyVarGen::from_bytes(bad_bytes);
        expect(!bad.public_key() && !bad.sign(rnd, m), "a generator that does not decode: refused");
        jjs::AffinePoint off{};
        off[0] = 1; off[32] = 1;                                          // (1, 1) is not on the curve
        expect(!jjs::SecretKeyVarGen(sk, off).public_key(), "a generator off the curve: refused");
        jjs::Scalar big;
        big.fill(0xFF);
        const auto batch = jjs::SecretKeyVarGen::sign_batch({{wire, rnd, m}, {bad, rnd, m}, {affine, rnd, m}, {affine, big, m}});
        expect(batch.size() == 4 && batch[0] && !batch[1] && batch[2] && !batch[3] && batch[0]->u == batch[2]->u && batch[0]->R == batch[2]->R,
               "sign_batch over both formats, with the refused items empty");
    }
    (void)pub; (void)signature;
    std::printf("SecretKeyVarGen, %s, %d failures\n", gpu ? "with the engine" : "host only", failures);
    return failures ? 1 : 0;
}

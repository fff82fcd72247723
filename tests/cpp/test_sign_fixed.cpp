// jjs::SecretKey (include/jjs_schnorr.hpp) on the reference's own bytes.  Input: a text file of hex lines -- "secret" (32:
// serde_secret_key), "public" (32: serde_public_key), "public_double" (64), "signature" (64: u || R compressed), "signature_double"
// (96), "m", "rnd" and "rnd_double" (32 each: the message and the nonce's RNG draws behind the two signatures).
// Without a second argument only what needs no engine runs: from_bytes / to_bytes and with_variable_generator.  With "gpu":
// public_key, public_key_double, sign, sign_double and the batches against the bytes, and refused items.
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
    if (argc < 2) { std::puts("usage: test_sign_fixed vector.txt [gpu]"); return 2; }
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
    const jjs::Scalar secret = arr<32>(f["secret"]), m = arr<32>(f["m"]), rnd = arr<32>(f["rnd"]), rnd_double = arr<32>(f["rnd_double"]);

    // ---- no engine ----
    const auto key = jjs::SecretKey::from_bytes(secret);
    expect(key && key->to_bytes() == secret && key->secret() == secret, "from_bytes / to_bytes round trip");
    // r = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7, little-endian
    const jjs::Scalar order = arr<32>(unhex("b72cf7d65e0e97d08210c8cc932068a6003b3401013b6706a9af3365eab47d0e"));
    jjs::Scalar below = order, above = order, big;
    below[0] -= 1; above[0] += 1; big.fill(0xFF);
    expect(!jjs::SecretKey::from_bytes(order) && !jjs::SecretKey::from_bytes(above) && !jjs::SecretKey::from_bytes(big), "from_bytes refuses r and beyond");
    expect(jjs::SecretKey::from_bytes(below) && jjs::SecretKey::from_bytes(jjs::Scalar{}), "from_bytes accepts r - 1 and 0");
    jjs::AffinePoint gen{};
    for (size_t i = 0; i < 64; ++i) gen[i] = (uint8_t)i;
    if (key) {
        const jjs::SecretKeyVarGen vg = key->with_variable_generator(gen);
        expect(vg.secret() == secret && vg.to_bytes() == jjs::SecretKeyVarGen(secret, gen).to_bytes(), "with_variable_generator is SecretKeyVarGen::new");
    }

    if (gpu && key) {
        jjs::Engine engine;
        const auto pk = key->public_key();
        expect(pk && compress(pk->as_ref()) == arr<32>(f["public"]), "public_key gives serde_public_key");
        const auto pkd = key->public_key_double();
        expect(pkd && compress(pkd->pk()) == arr<32>(f["public_double"]) && compress(pkd->pk_prime()) == arr<32>(f["public_double"], 32),
               "public_key_double gives serde_public_key_double");
        const auto sig = key->sign(rnd, m);
        expect(sig && sig->u == arr<32>(f["signature"]) && compress(sig->R) == arr<32>(f["signature"], 32), "sign gives serde_signature");
        expect(sig && pk && !pk->verify(*sig, m), "the signature verifies under the derived key");
        const auto sd = key->sign_double(rnd_double, m);
        expect(sd && sd->u == arr<32>(f["signature_double"]) && compress(sd->R) == arr<32>(f["signature_double"], 32) &&
                   compress(sd->R_prime) == arr<32>(f["signature_double"], 64), "sign_double gives serde_signature_double");
        expect(sd && pkd && !pkd->verify(*sd, m), "the double signature verifies under the derived key");
        const jjs::SecretKey bad(order);                                  // the constructor does not test the range: the engine does
        expect(!bad.public_key() && !bad.public_key_double() && !bad.sign(rnd, m) && !bad.sign_double(rnd, m), "sk = r: refused");
        expect(!key->sign(big, m) && !key->sign(rnd, big), "rnd or message out of range: refused");
        // a key per item, and one key for the call
        const auto mixed = jjs::SecretKey::sign_batch({{*key, rnd, m}, {bad, rnd, m}, {*key, big, m}, {*key, rnd, m}});
        expect(mixed.size() == 4 && mixed[0] && !mixed[1] && !mixed[2] && mixed[3] && sig && mixed[0]->u == sig->u && mixed[3]->R == sig->R,
               "sign_batch with a key per item, the refused items empty");
        const auto same = jjs::SecretKey::sign_batch({{*key, rnd, m}, {*key, big, m}, {*key, rnd, m}});
        expect(same.size() == 3 && same[0] && !same[1] && same[2] && sig && same[0]->u == sig->u && same[2]->R == sig->R,
               "sign_batch with one key for the call");
        const auto dsame = jjs::SecretKey::sign_double_batch({{*key, rnd_double, m}, {*key, rnd_double, m}});
        expect(dsame.size() == 2 && dsame[0] && dsame[1] && sd && dsame[1]->u == sd->u && dsame[1]->R_prime == sd->R_prime,
               "sign_double_batch with one key for the call");
        expect(jjs::SecretKey::sign_batch({}).empty(), "an empty batch");
    }
    std::printf("SecretKey, %s, %d failures\n", gpu ? "with the engine" : "host only", failures);
    return failures ? 1 : 0;
}

// Host-side mirror (C++17, header only) of the reference crate's verify interface, over the C ABI of
// jjs_gpu.h.  The reference is Rust and this image has no Rust toolchain, so this header plays the role
// of the shim in INTEGRATION.md: same type names, same method names, same argument meaning and the same
// error classes as
//   PublicKey::verify        /root/reference/src/keys/public.rs:114-135
//   PublicKeyDouble::verify  src/keys/public/double.rs:86-117
//   PublicKeyVarGen::verify  src/keys/public/var_gen.rs:107-133
//   Error                    src/error.rs:13-26
//   to_bytes / from_bytes    src/signatures.rs:101-119, src/keys/public.rs:80-94 (wire entry points)
// plus the batch entry points a GPU-backed crate would add (`verify_batch`, `verify_batch_bytes`).
// Points are held as affine canonical bytes (u || v): what `to_hash_inputs()` yields; `verify_batch_extended` takes
// them as the Rust `JubJubExtended` holds them (U || V || Z, normalised on the device: no host arithmetic).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "jjs_gpu.h"

namespace jjs {

using Scalar = std::array<uint8_t, 32>;     // JubJubScalar / BlsScalar: canonical little-endian
using AffinePoint = std::array<uint8_t, 64>;  // u || v
using ExtendedPoint = std::array<uint8_t, 96>;  // U || V || Z, affine point (U/Z, V/Z): get_u / get_v / get_z of JubJubExtended
using PointBytes = std::array<uint8_t, 32>;       // JubJubAffine::to_bytes / PublicKey::to_bytes: v with the parity of u in bit 255
using SignatureBytes = std::array<uint8_t, 64>;   // Signature::to_bytes: u || R
using BlsScalar = Scalar;
using JubJubScalar = Scalar;

// reference src/error.rs:13-26 (the variants reachable from verify) + the engine's own failures
// (InvalidMultisigTranscript and DuplicatedNonce, src/error.rs:23-24 and :27, are what multisig::sign_round_2 answers)
enum class Error { InvalidSignature, InvalidPoint, BytesError, Engine, InvalidMultisigTranscript, DuplicatedNonce };

inline const char* to_string(Error e) {
    switch (e) {
    case Error::InvalidSignature: return "Invalid Signature";   // src/error.rs:40-42
    case Error::InvalidPoint: return "Invalid Point";           // src/error.rs:43-45
    case Error::BytesError: return "InvalidData";
    case Error::InvalidMultisigTranscript: return "Invalid Multisig Transcript";
    case Error::DuplicatedNonce: return "Duplicated Nonce";
    default: return "engine error";
    }
}

// Result<(), Error>: empty optional == Ok(())
using VerifyResult = std::optional<Error>;

inline VerifyResult from_status(uint8_t s) {
    switch (s) {
    case JJS_STATUS_OK: return std::nullopt;
    case JJS_STATUS_INVALID_POINT: return Error::InvalidPoint;
    case JJS_STATUS_INVALID_SIGNATURE: return Error::InvalidSignature;
    default: return Error::BytesError;   // 3: an encoding the Rust from_bytes would have rejected
    }
}

struct EngineError : std::runtime_error {
    int code;
    EngineError(int c, const char* what) : std::runtime_error(std::string(what) + ": " + jjs_last_error()), code(c) {}
};

// RAII handle on the process-wide engine: device_count 1 = the current HIP device, k = devices 0..k-1,
// 0 = every visible device (batches of the host-buffer calls are then sharded across them).
class Engine {
  public:
    explicit Engine(int device_count = 1) { int rc = jjs_init(device_count); if (rc != JJS_OK) throw EngineError(rc, "jjs_init"); }
    int device_count() const { return jjs_device_count(); }
    // Pre-sizes the engine for verify_batch calls of at most `max_items` items of one scheme (JJS_SCHEME_*) and input format
    // (JJS_FORMAT_*): afterwards no such call allocates (include/jjs_gpu.h jjs_reserve).  The batch methods below are the
    // blocking host-buffer calls, hence host_buffers = 1.
    void reserve(int scheme, int format, size_t max_items) {
        int rc = jjs_reserve(scheme, format, max_items, 1);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_reserve");
    }
    // Waits for the device, then gives back what growth has retired and the key-table pools (jjs_trim).
    void trim() { int rc = jjs_trim(); if (rc != JJS_OK) throw EngineError(rc, "jjs_trim"); }
    ~Engine() { jjs_shutdown(); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
};

namespace detail {
// 16-byte aligned SoA staging buffer
class Soa {
  public:
    Soa(size_t items, size_t width) : width_(width), store_((items * width + 15) / 16 + 1) {}
    uint8_t* data() { return reinterpret_cast<uint8_t*>(store_.data()); }
    const uint8_t* data() const { return reinterpret_cast<const uint8_t*>(store_.data()); }
    template <size_t N>
    void put(size_t i, size_t off, const std::array<uint8_t, N>& v) { std::memcpy(data() + i * width_ + off, v.data(), N); }
  private:
    struct alignas(16) Block { uint8_t b[16]; };
    size_t width_;
    std::vector<Block> store_;
};
inline std::vector<VerifyResult> results(const std::vector<uint8_t>& status) {
    std::vector<VerifyResult> out;
    out.reserve(status.size());
    for (uint8_t s : status) out.push_back(from_status(s));
    return out;
}
}  // namespace detail

// The reference's serde form (src/serde_support.rs:21-46 and the same pattern for every type): a JSON
// string holding the base58 (Bitcoin alphabet) text of `to_bytes()`.  Decoding fails, like the reference's
// deserialiser, on a character outside the alphabet or a decoded length other than N.
namespace serde {
inline const char* alphabet() { return "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"; }
template <size_t N>
inline std::array<uint8_t, N> from_base58(const std::string& text) {
    std::vector<uint8_t> num;                       // big-endian base-256 digits, most significant first
    size_t zeros = 0;
    while (zeros < text.size() && text[zeros] == '1') ++zeros;
    for (char ch : text) {
        const char* pos = std::strchr(alphabet(), ch);
        if (!pos || ch == 0) throw std::invalid_argument("invalid base58 character");
        unsigned carry = (unsigned)(pos - alphabet());
        for (size_t i = num.size(); i-- > 0;) { carry += 58u * num[i]; num[i] = (uint8_t)carry; carry >>= 8; }
        while (carry) { num.insert(num.begin(), (uint8_t)carry); carry >>= 8; }
    }
    size_t lead = 0;
    while (lead < num.size() && num[lead] == 0) ++lead;
    if (zeros + (num.size() - lead) != N) throw std::invalid_argument("invalid length");
    std::array<uint8_t, N> out{};
    std::copy(num.begin() + lead, num.end(), out.begin() + zeros);
    return out;
}
template <size_t N>
inline std::string to_base58(const std::array<uint8_t, N>& bytes) {
    std::vector<uint8_t> digits;                    // base-58 digits, least significant first
    size_t zeros = 0;
    while (zeros < N && bytes[zeros] == 0) ++zeros;
    for (uint8_t b : bytes) {
        unsigned carry = b;
        for (auto& d : digits) { carry += 256u * d; d = (uint8_t)(carry % 58u); carry /= 58u; }
        while (carry) { digits.push_back((uint8_t)(carry % 58u)); carry /= 58u; }
    }
    std::string out(zeros, '1');
    for (size_t i = digits.size(); i-- > 0;) out.push_back(alphabet()[digits[i]]);
    return out;
}
}  // namespace serde

// `Signature { u, R }` (reference src/signatures.rs:62-65)
struct Signature {
    JubJubScalar u;
    AffinePoint R;
    bool is_valid() const;                 // Signature::is_valid (reference src/signatures.rs); see is_valid_batch below
};
// `SignatureDouble { u, R, R_prime }` (reference src/signatures/double.rs:66-70)
struct SignatureDouble {
    JubJubScalar u;
    AffinePoint R, R_prime;
    bool is_valid() const;                 // SignatureDouble::is_valid
};
// `SignatureVarGen { u, R }` (reference src/signatures/var_gen.rs)
struct SignatureVarGen {
    JubJubScalar u;
    AffinePoint R;
    bool is_valid() const;                 // SignatureVarGen::is_valid
};

// `PublicKey(JubJubExtended)` (reference src/keys/public.rs:52)
class PublicKey {
  public:
    explicit PublicKey(const AffinePoint& p) : point_(p) {}
    const AffinePoint& as_ref() const { return point_; }
    bool is_valid() const;                 // PublicKey::is_valid (reference src/keys/public.rs:159-164); see is_valid_batch below

    struct Item { AffinePoint pk; Signature sig; BlsScalar message; };   // (key point, signature, message)
    // PublicKey::verify (reference src/keys/public.rs:114-135)
    VerifyResult verify(const Signature& sig, const BlsScalar& message) const {
        return verify_batch({Item{point_, sig, message}})[0];
    }
    static std::vector<VerifyResult> verify_batch(const std::vector<Item>& items, uint64_t tally[4] = nullptr) {
        const size_t n = items.size();
        detail::Soa u(n, 32), r(n, 64), pk(n, 64), m(n, 32);
        for (size_t i = 0; i < n; ++i) {
            u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R);
            pk.put(i, 0, items[i].pk); m.put(i, 0, items[i].message);
        }
        std::vector<uint8_t> status(n);
        uint64_t t[4];
        int rc = jjs_verify_single(u.data(), r.data(), pk.data(), m.data(), n, status.data(), t);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_verify_single");
        if (tally) std::memcpy(tally, t, sizeof(t));
        return detail::results(status);
    }
    // The same with every point in extended coordinates: what `PublicKey::verify(&self, &Signature, BlsScalar)` holds
    // (reference src/keys/public.rs:114-118); the engine normalises on the device (jjs_verify_single_ext).
    struct ItemExtended { ExtendedPoint pk; JubJubScalar u; ExtendedPoint R; BlsScalar message; };
    static std::vector<VerifyResult> verify_batch_extended(const std::vector<ItemExtended>& items) {
        const size_t n = items.size();
        detail::Soa u(n, 32), r(n, 96), pk(n, 96), m(n, 32);
        for (size_t i = 0; i < n; ++i) {
            u.put(i, 0, items[i].u); r.put(i, 0, items[i].R); pk.put(i, 0, items[i].pk); m.put(i, 0, items[i].message);
        }
        std::vector<uint8_t> status(n);
        int rc = jjs_verify_single_ext(u.data(), r.data(), pk.data(), m.data(), n, status.data(), nullptr);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_verify_single_ext");
        return detail::results(status);
    }
    // Batch verify straight from the reference's wire formats (`Signature::to_bytes` 64 B = u || R,
    // `PublicKey::to_bytes` 32 B; reference src/signatures.rs:101-119, src/keys/public.rs:80-94): points are
    // decompressed on the device; an undecodable item yields Error::BytesError, as `from_bytes` would.
    struct ItemBytes { std::array<uint8_t, 32> pk; std::array<uint8_t, 64> sig; BlsScalar message; };
    static std::vector<VerifyResult> verify_batch_bytes(const std::vector<ItemBytes>& items) {
        const size_t n = items.size();
        detail::Soa sig(n, 64), pk(n, 32), m(n, 32);
        for (size_t i = 0; i < n; ++i) { sig.put(i, 0, items[i].sig); pk.put(i, 0, items[i].pk); m.put(i, 0, items[i].message); }
        std::vector<uint8_t> status(n);
        int rc = jjs_verify_single_wire(sig.data(), pk.data(), m.data(), n, status.data(), nullptr);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_verify_single_wire");
        return detail::results(status);
    }
  private:
    AffinePoint point_;
};

// `PublicKeyDouble(pk, pk_prime)` (reference src/keys/public/double.rs:45)
class PublicKeyDouble {
  public:
    PublicKeyDouble(const AffinePoint& pk, const AffinePoint& pk_prime) : pk_(pk), pk_prime_(pk_prime) {}
    const AffinePoint& pk() const { return pk_; }
    const AffinePoint& pk_prime() const { return pk_prime_; }
    bool is_valid() const;                 // PublicKeyDouble::is_valid

    struct Item { AffinePoint pk, pk_prime; SignatureDouble sig; BlsScalar message; };
    // PublicKeyDouble::verify (reference src/keys/public/double.rs:86-117)
    VerifyResult verify(const SignatureDouble& sig, const BlsScalar& message) const {
        return verify_batch({Item{pk_, pk_prime_, sig, message}})[0];
    }
    static std::vector<VerifyResult> verify_batch(const std::vector<Item>& items) {
        const size_t n = items.size();
        detail::Soa u(n, 32), r(n, 64), rp(n, 64), pk(n, 64), pkp(n, 64), m(n, 32);
        for (size_t i = 0; i < n; ++i) {
            u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R); rp.put(i, 0, items[i].sig.R_prime);
            pk.put(i, 0, items[i].pk); pkp.put(i, 0, items[i].pk_prime); m.put(i, 0, items[i].message);
        }
        std::vector<uint8_t> status(n);
        int rc = jjs_verify_double(u.data(), r.data(), rp.data(), pk.data(), pkp.data(), m.data(), n, status.data(), nullptr);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_verify_double");
        return detail::results(status);
    }
  private:
    AffinePoint pk_, pk_prime_;
};

// `PublicKeyVarGen { pk, generator }` (reference src/keys/public/var_gen.rs:40-43)
class PublicKeyVarGen {
  public:
    PublicKeyVarGen(const AffinePoint& pk, const AffinePoint& generator) : pk_(pk), generator_(generator) {}
    const AffinePoint& public_key() const { return pk_; }
    const AffinePoint& generator() const { return generator_; }
    bool is_valid() const;                 // PublicKeyVarGen::is_valid

    struct Item { AffinePoint pk, generator; SignatureVarGen sig; BlsScalar message; };
    // PublicKeyVarGen::verify (reference src/keys/public/var_gen.rs:107-133)
    VerifyResult verify(const SignatureVarGen& sig, const BlsScalar& message) const {
        return verify_batch({Item{pk_, generator_, sig, message}})[0];
    }
    static std::vector<VerifyResult> verify_batch(const std::vector<Item>& items) {
        const size_t n = items.size();
        detail::Soa u(n, 32), r(n, 64), pk(n, 64), gen(n, 64), m(n, 32);
        for (size_t i = 0; i < n; ++i) {
            u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R);
            pk.put(i, 0, items[i].pk); gen.put(i, 0, items[i].generator); m.put(i, 0, items[i].message);
        }
        std::vector<uint8_t> status(n);
        int rc = jjs_verify_vargen(u.data(), r.data(), pk.data(), gen.data(), m.data(), n, status.data(), nullptr);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_verify_vargen");
        return detail::results(status);
    }
  private:
    AffinePoint pk_, generator_;
};

// `SecretKeyVarGen { sk, generator }` (reference src/keys/secret/var_gen.rs:98-101) with the generator as a POINT, as `new` (:147),
// `SecretKey::with_variable_generator` and `from_bytes` (:109-131) take it: affine u || v, or the 32 bytes of JubJubAffine::to_bytes,
// which go to the device as they are (jjs_sign_vargen_pt, jjs_public_keys_vargen).  A generator of test and benchmark material like
// every signer of the engine, NOT constant time: never use with production keys.  An empty optional is the engine's status 3, the
// reference's BytesError: sk or rnd >= r, message >= q, or a generator that is not canonical, does not decode or is off the curve.
class SecretKeyVarGen {
  public:
    SecretKeyVarGen(const JubJubScalar& sk, const AffinePoint& generator) : sk_(sk), gen_(generator), wire_(false) {}     // SecretKeyVarGen::new
    static SecretKeyVarGen from_bytes(const std::array<uint8_t, 64>& bytes) {      // sk || generator compressed; nothing is decoded here
        SecretKeyVarGen k(JubJubScalar{}, AffinePoint{});
        std::memcpy(k.sk_.data(), bytes.data(), 32);
        std::memcpy(k.gen_.data(), bytes.data() + 32, 32);
        k.wire_ = true;
        return k;
    }
    std::array<uint8_t, 64> to_bytes() const {
        std::array<uint8_t, 64> out{};
        std::memcpy(out.data(), sk_.data(), 32);
        std::memcpy(out.data() + 32, gen_.data() + (wire_ ? 0 : 32), 32);
        if (!wire_) out[63] |= (uint8_t)((gen_[0] & 1) << 7);               // v with the parity of u in bit 255
        return out;
    }
    const JubJubScalar& secret() const { return sk_; }
    // PublicKeyVarGen::from(&SecretKeyVarGen): pk = sk * generator
    std::optional<PublicKeyVarGen> public_key() const {
        AffinePoint pk{}, gen{};
        uint8_t status = 0;
        int rc = jjs_public_keys_vargen(format(), sk_.data(), gen_.data(), 1, 1, pk.data(), gen.data(), &status);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_public_keys_vargen");
        if (status != JJS_STATUS_OK) return std::nullopt;
        return PublicKeyVarGen(pk, gen);
    }
    // SecretKeyVarGen::sign (:228-256) given the RNG draw `rnd` that the hedged nonce mixes in
    std::optional<SignatureVarGen> sign(const JubJubScalar& rnd, const BlsScalar& message) const;
    struct Item;
    static std::vector<std::optional<SignatureVarGen>> sign_batch(const std::vector<Item>& items);
  private:
    int format() const { return wire_ ? JJS_FORMAT_WIRE : JJS_FORMAT_AFFINE; }
    JubJubScalar sk_;
    AffinePoint gen_;                      // a wire generator: its 32 bytes, then zeros
    bool wire_;
};
struct SecretKeyVarGen::Item { SecretKeyVarGen key; JubJubScalar rnd; BlsScalar message; };
// one call per generator format among the items (the host-buffer call asks no alignment)
inline std::vector<std::optional<SignatureVarGen>> SecretKeyVarGen::sign_batch(const std::vector<Item>& items) {
    std::vector<std::optional<SignatureVarGen>> out(items.size());
    for (int wire = 0; wire < 2; ++wire) {
        std::vector<size_t> idx;
        for (size_t i = 0; i < items.size(); ++i)
            if ((int)items[i].key.wire_ == wire) idx.push_back(i);
        const size_t n = idx.size(), w = wire ? 32 : 64;
        if (!n) continue;
        std::vector<uint8_t> sk(n * 32), gen(n * w), rnd(n * 32), m(n * 32), u(n * 32), R(n * 64), status(n);
        for (size_t j = 0; j < n; ++j) {
            const Item& it = items[idx[j]];
            std::memcpy(&sk[32 * j], it.key.sk_.data(), 32); std::memcpy(&gen[w * j], it.key.gen_.data(), w);
            std::memcpy(&rnd[32 * j], it.rnd.data(), 32); std::memcpy(&m[32 * j], it.message.data(), 32);
        }
        int rc = jjs_sign_vargen_pt(wire ? JJS_FORMAT_WIRE : JJS_FORMAT_AFFINE, sk.data(), gen.data(), n, rnd.data(), m.data(), n, u.data(), R.data(),
                                    nullptr, nullptr, status.data());
        if (rc != JJS_OK) throw EngineError(rc, "jjs_sign_vargen_pt");
        for (size_t j = 0; j < n; ++j) {
            if (status[j] != JJS_STATUS_OK) continue;
            SignatureVarGen s;
            std::memcpy(s.u.data(), &u[32 * j], 32); std::memcpy(s.R.data(), &R[64 * j], 64);
            out[idx[j]] = s;
        }
    }
    return out;
}
inline std::optional<SignatureVarGen> SecretKeyVarGen::sign(const JubJubScalar& rnd, const BlsScalar& message) const {
    return sign_batch({Item{*this, rnd, message}})[0];
}
// `SecretKey::with_variable_generator(generator)` from the bare scalar (SecretKey below has it as a member)
inline SecretKeyVarGen with_variable_generator(const JubJubScalar& sk, const AffinePoint& generator) { return SecretKeyVarGen(sk, generator); }

// `SecretKey(JubJubScalar)` (reference src/keys/secret.rs) in the single and the double scheme: the 32 little-endian bytes of the
// scalar, through the blocking host-buffer calls jjs_sign_fixed and jjs_public_keys_fixed.  A generator of test and benchmark
// material like every signer of the engine, NOT constant time: never use with production keys.  An empty optional is the engine's
// status 3, the reference's BytesError: sk or rnd >= r, or message >= q.
class SecretKey {
  public:
    explicit SecretKey(const JubJubScalar& sk) : sk_(sk) {}
    // SecretKey::from_bytes (:120-126): empty for a scalar that is not below the group order (a compare on the host)
    static std::optional<SecretKey> from_bytes(const std::array<uint8_t, 32>& bytes) {
        static const uint8_t order_be[32] = {0x0E, 0x7D, 0xB4, 0xEA, 0x65, 0x33, 0xAF, 0xA9, 0x06, 0x67, 0x3B, 0x01, 0x01, 0x34, 0x3B, 0x00,
                                             0xA6, 0x68, 0x20, 0x93, 0xCC, 0xC8, 0x10, 0x82, 0xD0, 0x97, 0x0E, 0x5E, 0xD6, 0xF7, 0x2C, 0xB7};
        for (int i = 0; i < 32; ++i) {
            if (bytes[31 - i] < order_be[i]) return SecretKey(bytes);
            if (bytes[31 - i] > order_be[i]) return std::nullopt;
        }
        return std::nullopt;
    }
    std::array<uint8_t, 32> to_bytes() const { return sk_; }
    const JubJubScalar& secret() const { return sk_; }
    // PublicKey::from(&SecretKey): sk * G
    std::optional<PublicKey> public_key() const {
        AffinePoint pk{};
        uint8_t status = 0;
        int rc = jjs_public_keys_fixed(JJS_SCHEME_SINGLE, sk_.data(), 1, pk.data(), nullptr, nullptr, &status);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_public_keys_fixed");
        if (status != JJS_STATUS_OK) return std::nullopt;
        return PublicKey(pk);
    }
    // PublicKeyDouble::from(&SecretKey): (sk * G, sk * G')
    std::optional<PublicKeyDouble> public_key_double() const {
        AffinePoint pk{}, pkp{};
        uint8_t status = 0;
        int rc = jjs_public_keys_fixed(JJS_SCHEME_DOUBLE, sk_.data(), 1, pk.data(), pkp.data(), nullptr, &status);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_public_keys_fixed");
        if (status != JJS_STATUS_OK) return std::nullopt;
        return PublicKeyDouble(pk, pkp);
    }
    struct Item;
    // SecretKey::sign (:174-194) and sign_double (src/keys/secret/double.rs:56-85) given the RNG draw `rnd` that the hedged nonce mixes in
    std::optional<Signature> sign(const JubJubScalar& rnd, const BlsScalar& message) const;
    std::optional<SignatureDouble> sign_double(const JubJubScalar& rnd, const BlsScalar& message) const;
    // one call per batch; with one key for the call (n_sk = 1) when every item holds the same key
    static std::vector<std::optional<Signature>> sign_batch(const std::vector<Item>& items);
    static std::vector<std::optional<SignatureDouble>> sign_double_batch(const std::vector<Item>& items);
    // SecretKey::with_variable_generator (src/keys/secret/var_gen.rs:34-41)
    SecretKeyVarGen with_variable_generator(const AffinePoint& generator) const { return SecretKeyVarGen(sk_, generator); }
  private:
    struct Columns { std::vector<uint8_t> u, R, Rp, status; };
    static Columns sign_columns(int scheme, const std::vector<Item>& items);
    JubJubScalar sk_;
};
struct SecretKey::Item { SecretKey key; JubJubScalar rnd; BlsScalar message; };
inline SecretKey::Columns SecretKey::sign_columns(int scheme, const std::vector<Item>& items) {
    const size_t n = items.size();
    bool one = n > 1;
    for (size_t i = 1; i < n && one; ++i) one = items[i].key.sk_ == items[0].key.sk_;
    const size_t n_sk = one ? 1 : n;
    const bool dbl = scheme == JJS_SCHEME_DOUBLE;
    std::vector<uint8_t> sk(n_sk * 32), rnd(n * 32), m(n * 32);
    Columns c{std::vector<uint8_t>(n * 32), std::vector<uint8_t>(n * 64), std::vector<uint8_t>(dbl ? n * 64 : 0), std::vector<uint8_t>(n)};
    for (size_t i = 0; i < n; ++i) {
        if (i < n_sk) std::memcpy(&sk[32 * i], items[i].key.sk_.data(), 32);
        std::memcpy(&rnd[32 * i], items[i].rnd.data(), 32); std::memcpy(&m[32 * i], items[i].message.data(), 32);
    }
    int rc = jjs_sign_fixed(scheme, sk.data(), n_sk, rnd.data(), m.data(), n, c.u.data(), c.R.data(), dbl ? c.Rp.data() : nullptr, nullptr, nullptr,
                            nullptr, nullptr, c.status.data());
    if (rc != JJS_OK) throw EngineError(rc, "jjs_sign_fixed");
    return c;
}
inline std::vector<std::optional<Signature>> SecretKey::sign_batch(const std::vector<Item>& items) {
    std::vector<std::optional<Signature>> out(items.size());
    if (items.empty()) return out;
    const Columns c = sign_columns(JJS_SCHEME_SINGLE, items);
    for (size_t i = 0; i < items.size(); ++i) {
        if (c.status[i] != JJS_STATUS_OK) continue;
        Signature s;
        std::memcpy(s.u.data(), &c.u[32 * i], 32); std::memcpy(s.R.data(), &c.R[64 * i], 64);
        out[i] = s;
    }
    return out;
}
inline std::vector<std::optional<SignatureDouble>> SecretKey::sign_double_batch(const std::vector<Item>& items) {
    std::vector<std::optional<SignatureDouble>> out(items.size());
    if (items.empty()) return out;
    const Columns c = sign_columns(JJS_SCHEME_DOUBLE, items);
    for (size_t i = 0; i < items.size(); ++i) {
        if (c.status[i] != JJS_STATUS_OK) continue;
        SignatureDouble s;
        std::memcpy(s.u.data(), &c.u[32 * i], 32); std::memcpy(s.R.data(), &c.R[64 * i], 64); std::memcpy(s.R_prime.data(), &c.Rp[64 * i], 64);
        out[i] = s;
    }
    return out;
}
inline std::optional<Signature> SecretKey::sign(const JubJubScalar& rnd, const BlsScalar& message) const {
    return sign_batch({Item{*this, rnd, message}})[0];
}
inline std::optional<SignatureDouble> SecretKey::sign_double(const JubJubScalar& rnd, const BlsScalar& message) const {
    return sign_double_batch({Item{*this, rnd, message}})[0];
}

// `is_valid` alone (include/jjs_gpu.h jjs_keys_check / jjs_signatures_check): one bool per key or signature -- every point on
// the curve, not the identity and torsion-free -- without verifying anything; a malformed encoding (a coordinate >= q, a scalar
// >= r, bytes `from_bytes` refuses) is not valid.  Blocking host-buffer calls.  The ExtendedPoint and PointBytes forms take
// single-point keys as the Rust types hold them (`JubJubExtended`) and as they travel (`PublicKey::to_bytes`); `affine_out`
// (optional) receives the canonical affine points, zero bytes for a malformed one: the bulk `to_hash_inputs` / `from_bytes`.
namespace detail {
inline std::vector<bool> valid_of(int rc, const std::vector<uint8_t>& status, const char* what) {
    if (rc != JJS_OK) throw EngineError(rc, what);
    std::vector<bool> out(status.size());
    for (size_t i = 0; i < status.size(); ++i) out[i] = status[i] == JJS_STATUS_OK;
    return out;
}
template <size_t W>
inline std::vector<bool> keys_valid(int format, const std::vector<std::array<uint8_t, W>>& keys, std::vector<AffinePoint>* affine_out) {
    const size_t n = keys.size();
    Soa k(n, W), a(affine_out ? n : 0, 64);
    for (size_t i = 0; i < n; ++i) k.put(i, 0, keys[i]);
    std::vector<uint8_t> status(n);
    const int rc = jjs_keys_check(JJS_SCHEME_SINGLE, format, k.data(), nullptr, n, status.data(), nullptr, affine_out ? a.data() : nullptr, nullptr);
    if (affine_out && rc == JJS_OK) {
        affine_out->resize(n);
        for (size_t i = 0; i < n; ++i) std::memcpy((*affine_out)[i].data(), a.data() + 64 * i, 64);
    }
    return valid_of(rc, status, "jjs_keys_check");
}
}  // namespace detail
inline std::vector<bool> is_valid_batch(const std::vector<PublicKey>& keys) {
    const size_t n = keys.size();
    detail::Soa k(n, 64);
    for (size_t i = 0; i < n; ++i) k.put(i, 0, keys[i].as_ref());
    std::vector<uint8_t> status(n);
    return detail::valid_of(jjs_keys_check(JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, k.data(), nullptr, n, status.data(), nullptr, nullptr, nullptr),
                            status, "jjs_keys_check");
}
inline std::vector<bool> is_valid_batch(const std::vector<PublicKeyDouble>& keys) {
    const size_t n = keys.size();
    detail::Soa k(n, 64), kp(n, 64);
    for (size_t i = 0; i < n; ++i) { k.put(i, 0, keys[i].pk()); kp.put(i, 0, keys[i].pk_prime()); }
    std::vector<uint8_t> status(n);
    return detail::valid_of(jjs_keys_check(JJS_SCHEME_DOUBLE, JJS_FORMAT_AFFINE, k.data(), kp.data(), n, status.data(), nullptr, nullptr, nullptr),
                            status, "jjs_keys_check");
}
inline std::vector<bool> is_valid_batch(const std::vector<PublicKeyVarGen>& keys) {
    const size_t n = keys.size();
    detail::Soa k(n, 64), gen(n, 64);
    for (size_t i = 0; i < n; ++i) { k.put(i, 0, keys[i].public_key()); gen.put(i, 0, keys[i].generator()); }
    std::vector<uint8_t> status(n);
    return detail::valid_of(jjs_keys_check(JJS_SCHEME_VARGEN, JJS_FORMAT_AFFINE, k.data(), gen.data(), n, status.data(), nullptr, nullptr, nullptr),
                            status, "jjs_keys_check");
}
inline std::vector<bool> is_valid_batch(const std::vector<ExtendedPoint>& keys, std::vector<AffinePoint>* affine_out = nullptr) {
    return detail::keys_valid<96>(JJS_FORMAT_EXT, keys, affine_out);
}
inline std::vector<bool> is_valid_batch(const std::vector<PointBytes>& keys, std::vector<AffinePoint>* affine_out = nullptr) {
    return detail::keys_valid<32>(JJS_FORMAT_WIRE, keys, affine_out);
}
inline std::vector<bool> is_valid_batch(const std::vector<Signature>& sigs) {
    const size_t n = sigs.size();
    detail::Soa u(n, 32), r(n, 64);
    for (size_t i = 0; i < n; ++i) { u.put(i, 0, sigs[i].u); r.put(i, 0, sigs[i].R); }
    std::vector<uint8_t> status(n);
    return detail::valid_of(jjs_signatures_check(JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, u.data(), r.data(), nullptr, n, status.data(), nullptr,
                                                 nullptr, nullptr, nullptr), status, "jjs_signatures_check");
}
inline std::vector<bool> is_valid_batch(const std::vector<SignatureDouble>& sigs) {
    const size_t n = sigs.size();
    detail::Soa u(n, 32), r(n, 64), rp(n, 64);
    for (size_t i = 0; i < n; ++i) { u.put(i, 0, sigs[i].u); r.put(i, 0, sigs[i].R); rp.put(i, 0, sigs[i].R_prime); }
    std::vector<uint8_t> status(n);
    return detail::valid_of(jjs_signatures_check(JJS_SCHEME_DOUBLE, JJS_FORMAT_AFFINE, u.data(), r.data(), rp.data(), n, status.data(), nullptr,
                                                 nullptr, nullptr, nullptr), status, "jjs_signatures_check");
}
inline std::vector<bool> is_valid_batch(const std::vector<SignatureVarGen>& sigs) {
    const size_t n = sigs.size();
    detail::Soa u(n, 32), r(n, 64);
    for (size_t i = 0; i < n; ++i) { u.put(i, 0, sigs[i].u); r.put(i, 0, sigs[i].R); }
    std::vector<uint8_t> status(n);
    return detail::valid_of(jjs_signatures_check(JJS_SCHEME_VARGEN, JJS_FORMAT_AFFINE, u.data(), r.data(), nullptr, n, status.data(), nullptr,
                                                 nullptr, nullptr, nullptr), status, "jjs_signatures_check");
}
inline bool Signature::is_valid() const { return is_valid_batch(std::vector<Signature>{*this})[0]; }
inline bool SignatureDouble::is_valid() const { return is_valid_batch(std::vector<SignatureDouble>{*this})[0]; }
inline bool SignatureVarGen::is_valid() const { return is_valid_batch(std::vector<SignatureVarGen>{*this})[0]; }
inline bool PublicKey::is_valid() const { return is_valid_batch(std::vector<PublicKey>{*this})[0]; }
inline bool PublicKeyDouble::is_valid() const { return is_valid_batch(std::vector<PublicKeyDouble>{*this})[0]; }
inline bool PublicKeyVarGen::is_valid() const { return is_valid_batch(std::vector<PublicKeyVarGen>{*this})[0]; }

// One verdict per batch (include/jjs_gpu.h jjs_verify_all_*): true when every item would verify.  `status` (optional)
// receives the statuses of verify_batch when the verdict is false.
namespace detail {
inline bool verdict(int rc, int v, const char* what) {
    if (rc != JJS_OK) throw EngineError(rc, what);
    return v == 1;
}
}  // namespace detail
inline bool verify_all_single(const std::vector<PublicKey::Item>& items, std::vector<VerifyResult>* status = nullptr) {
    const size_t n = items.size();
    detail::Soa u(n, 32), r(n, 64), pk(n, 64), m(n, 32);
    for (size_t i = 0; i < n; ++i) {
        u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R); pk.put(i, 0, items[i].pk); m.put(i, 0, items[i].message);
    }
    std::vector<uint8_t> st(status ? n : 0);
    int v = 0;
    const bool ok = detail::verdict(jjs_verify_all_single(u.data(), r.data(), pk.data(), m.data(), n, status ? st.data() : nullptr, &v),
                                    v, "jjs_verify_all_single");
    if (status) *status = detail::results(st);
    return ok;
}
inline bool verify_all_double(const std::vector<PublicKeyDouble::Item>& items, std::vector<VerifyResult>* status = nullptr) {
    const size_t n = items.size();
    detail::Soa u(n, 32), r(n, 64), rp(n, 64), pk(n, 64), pkp(n, 64), m(n, 32);
    for (size_t i = 0; i < n; ++i) {
        u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R); rp.put(i, 0, items[i].sig.R_prime);
        pk.put(i, 0, items[i].pk); pkp.put(i, 0, items[i].pk_prime); m.put(i, 0, items[i].message);
    }
    std::vector<uint8_t> st(status ? n : 0);
    int v = 0;
    const bool ok = detail::verdict(jjs_verify_all_double(u.data(), r.data(), rp.data(), pk.data(), pkp.data(), m.data(), n,
                                                          status ? st.data() : nullptr, &v), v, "jjs_verify_all_double");
    if (status) *status = detail::results(st);
    return ok;
}
inline bool verify_all_vargen(const std::vector<PublicKeyVarGen::Item>& items, std::vector<VerifyResult>* status = nullptr) {
    const size_t n = items.size();
    detail::Soa u(n, 32), r(n, 64), pk(n, 64), gen(n, 64), m(n, 32);
    for (size_t i = 0; i < n; ++i) {
        u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R); pk.put(i, 0, items[i].pk);
        gen.put(i, 0, items[i].generator); m.put(i, 0, items[i].message);
    }
    std::vector<uint8_t> st(status ? n : 0);
    int v = 0;
    const bool ok = detail::verdict(jjs_verify_all_vargen(u.data(), r.data(), pk.data(), gen.data(), m.data(), n,
                                                          status ? st.data() : nullptr, &v), v, "jjs_verify_all_vargen");
    if (status) *status = detail::results(st);
    return ok;
}

// Registered key sets (include/jjs_gpu.h jjs_keyset_*): keys validated and tabled once on the device, then verified against by
// index.  Move-only; the destructor destroys the set (calls already queued on a stream still complete).
namespace multisig { struct CombineResult; struct CombineError; }
class KeySet {
  public:
    // raw form: scheme JJS_SCHEME_*, key format JJS_FORMAT_* and the key columns of jjs_keyset_create
    KeySet(int scheme, int format, const uint8_t* keys, const uint8_t* keys2, size_t n_keys) : scheme_(scheme), status_(n_keys) {
        int rc = jjs_keyset_create(scheme, format, keys, keys2, n_keys, status_.data(), &handle_);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_create");
    }
    explicit KeySet(const std::vector<PublicKey>& keys) : KeySet(JJS_SCHEME_SINGLE, column(keys, [](const PublicKey& k) { return k.as_ref(); }), keys.size()) {}
    explicit KeySet(const std::vector<PublicKeyDouble>& keys)
        : KeySet(JJS_SCHEME_DOUBLE, column(keys, [](const PublicKeyDouble& k) { return k.pk(); }),
                 column(keys, [](const PublicKeyDouble& k) { return k.pk_prime(); }), keys.size()) {}
    explicit KeySet(const std::vector<PublicKeyVarGen>& keys)
        : KeySet(JJS_SCHEME_VARGEN, column(keys, [](const PublicKeyVarGen& k) { return k.public_key(); }),
                 column(keys, [](const PublicKeyVarGen& k) { return k.generator(); }), keys.size()) {}
    KeySet(KeySet&& o) noexcept : scheme_(o.scheme_), handle_(o.handle_), status_(std::move(o.status_)) { o.handle_ = 0; }
    KeySet& operator=(KeySet&& o) noexcept {
        if (this != &o) { reset(); scheme_ = o.scheme_; handle_ = o.handle_; status_ = std::move(o.status_); o.handle_ = 0; }
        return *this;
    }
    KeySet(const KeySet&) = delete;
    KeySet& operator=(const KeySet&) = delete;
    ~KeySet() { reset(); }

    jjs_keyset handle() const { return handle_; }
    // per key: 0 valid, 1 not `is_valid`, 3 malformed
    const std::vector<uint8_t>& key_status() const { return status_; }
    std::array<uint64_t, JJS_KEYSET_INFO> info() const {
        std::array<uint64_t, JJS_KEYSET_INFO> out{};
        int rc = jjs_keyset_info(handle_, out.data());
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_info");
        return out;
    }
    // raw form: the signature columns of jjs_keyset_verify for `format`; blocking
    void verify(int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, const uint8_t* m, size_t n,
                uint8_t* status, uint64_t tally[4] = nullptr) const {
        int rc = jjs_keyset_verify(handle_, format, key_idx, s0, s1, s2, m, n, status, tally);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_verify");
    }
    // BY KEY (jjs_keyset_find, jjs_keyset_verify_keys): K0, K1 are the key columns of the inline call of the set's scheme in
    // `format`.  find: idx_out[i] = the index of item i's key, or 0xFFFFFFFF -- what verify(), verify_all() and the multisig_*
    // calls take as key_idx.  verify_keys: status and tally of the inline call on the same columns, whatever the set holds (items
    // whose key is not registered are verified inline); idx_out (nullable) tells which were found.  Host buffers, blocking.
    void find(int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint32_t* idx_out) const {
        int rc = jjs_keyset_find(handle_, format, K0, K1, n, idx_out);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_find");
    }
    void verify_keys(int format, const uint8_t* K0, const uint8_t* K1, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2,
                     const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4] = nullptr, uint32_t* idx_out = nullptr) const {
        int rc = jjs_keyset_verify_keys(handle_, format, K0, K1, s0, s1, s2, m, n, status, tally, idx_out);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_verify_keys");
    }
    // `PublicKey::verify(&self, &Signature, BlsScalar)` in its batch form against a set of PublicKey: the results of
    // PublicKey::verify_batch(items), with the registered keys' tables where an item's key is in the set
    std::vector<VerifyResult> verify(const std::vector<PublicKey::Item>& items, uint64_t tally[4] = nullptr) const {
        if (scheme_ != JJS_SCHEME_SINGLE) throw std::invalid_argument("PublicKey items need a key set of PublicKey");
        const size_t n = items.size();
        detail::Soa u(n, 32), r(n, 64), pk(n, 64), m(n, 32);
        for (size_t i = 0; i < n; ++i) {
            u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R);
            pk.put(i, 0, items[i].pk); m.put(i, 0, items[i].message);
        }
        std::vector<uint8_t> status(n);
        verify_keys(JJS_FORMAT_AFFINE, pk.data(), nullptr, u.data(), r.data(), nullptr, m.data(), n, status.data(), tally);
        return detail::results(status);
    }
    // the index of every key in the set (0xFFFFFFFF: not registered)
    std::vector<uint32_t> find(const std::vector<PublicKey>& keys) const {
        if (scheme_ != JJS_SCHEME_SINGLE) throw std::invalid_argument("PublicKey queries need a key set of PublicKey");
        std::vector<uint32_t> idx(keys.size());
        const detail::Soa c = column(keys, [](const PublicKey& k) { return k.as_ref(); });
        find(JJS_FORMAT_AFFINE, c.data(), nullptr, keys.size(), idx.data());
        return idx;
    }
    // ADDING KEYS to the live set (jjs_keyset_add): keys, keys2 and format as the raw constructor takes them.  Appended, candidate
    // i is registered at index n_old + i whatever it is; with `unique` a candidate the set (or an earlier candidate) already holds
    // gets that index and a malformed one 0xFFFFFFFF.  Old indices never change; calls from other threads go on meanwhile.
    // key_status() follows the set.  Host buffers, blocking.
    struct Added {
        std::vector<uint32_t> idx;            // per candidate: the index its key is registered at
        std::vector<uint8_t> key_status;      // per candidate: 0 valid, 1 not `is_valid`, 3 malformed
        size_t n_added = 0;                   // keys the set gained
    };
    Added add(int format, const uint8_t* keys, const uint8_t* keys2, size_t n, bool unique = false) {
        Added a;
        a.idx.resize(n); a.key_status.resize(n);
        int rc = jjs_keyset_add(handle_, format, keys, keys2, n, unique ? JJS_KEYSET_ADD_UNIQUE : JJS_KEYSET_ADD_APPEND, a.key_status.data(),
                                a.idx.data(), &a.n_added);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_add");
        for (size_t i = 0; i < n; ++i) {
            if (a.idx[i] == 0xFFFFFFFFu || a.idx[i] < status_.size()) continue;
            status_.resize((size_t)a.idx[i] + 1);
            status_[a.idx[i]] = a.key_status[i];
        }
        return a;
    }
    Added add(const std::vector<PublicKey>& keys, bool unique = false) {
        if (scheme_ != JJS_SCHEME_SINGLE) throw std::invalid_argument("PublicKey candidates need a key set of PublicKey");
        const detail::Soa c = column(keys, [](const PublicKey& k) { return k.as_ref(); });
        return add(JJS_FORMAT_AFFINE, c.data(), nullptr, keys.size(), unique);
    }
    // room for n_keys_total keys in all (jjs_keyset_reserve): the adds up to there move nothing
    void reserve(size_t n_keys_total) {
        int rc = jjs_keyset_reserve(handle_, n_keys_total);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_reserve");
    }
    std::array<uint64_t, JJS_KEYSET_GROWTH> growth() const {
        std::array<uint64_t, JJS_KEYSET_GROWTH> out{};
        int rc = jjs_keyset_growth(handle_, out.data());
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_growth");
        return out;
    }
    // REMOVING KEYS from the live set (jjs_keyset_remove), in place: no index moves, a removed index verifies nothing (status 3)
    // and its key is found nowhere.  key_status() becomes 3 at removed indices.  Host buffers, blocking.
    struct Removed {
        std::vector<uint8_t> result;          // per index: the key's status before the call, JJS_KEY_WAS_REMOVED or JJS_KEY_NOT_IN_RANGE
        size_t n_removed = 0;                 // distinct indices this call removed
    };
    Removed remove(const std::vector<uint32_t>& idx) {
        Removed r;
        r.result.resize(idx.size());
        int rc = jjs_keyset_remove(handle_, idx.data(), idx.size(), r.result.data(), &r.n_removed);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_remove");
        for (uint32_t i : idx)
            if (i < status_.size()) status_[i] = 3;
        return r;
    }
    // Drops the removed keys (jjs_keyset_compact): the set becomes the set of the survivors in their order, in a new allocation.
    // EVERY INDEX CHANGES: returns the map, map[i] the new index of old index i, 0xFFFFFFFF for a removed one; quiescing the
    // callers that still hold old indices is the caller's business.  key_status() follows.
    std::vector<uint32_t> compact() {
        std::vector<uint32_t> map(status_.size());
        size_t n_new = 0;
        int rc = jjs_keyset_compact(handle_, map.data(), map.size(), &n_new);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_compact");
        std::vector<uint8_t> kept(n_new);
        for (size_t i = 0; i < map.size(); ++i)
            if (map[i] != 0xFFFFFFFFu) kept[map[i]] = status_[i];
        status_.swap(kept);
        return map;
    }
    std::array<uint64_t, JJS_KEYSET_REMOVAL> removal() const {
        std::array<uint64_t, JJS_KEYSET_REMOVAL> out{};
        int rc = jjs_keyset_removal(handle_, out.data());
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_removal");
        return out;
    }
    // one verdict for the batch (jjs_keyset_verify_all): true when every item verifies; `status` (nullable, n bytes) holds
    // the statuses of verify() when the verdict is false and is all zero otherwise
    bool verify_all(int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, const uint8_t* m, size_t n,
                    uint8_t* status = nullptr) const {
        int verdict = 0;
        int rc = jjs_keyset_verify_all(handle_, format, key_idx, s0, s1, s2, m, n, status, &verdict);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_keyset_verify_all");
        return verdict == 1;
    }
    // raw form of the multisignature call against the set (jjs_multisig_combine_keyset): host buffers, blocking; the columns and
    // outputs of jjs_multisig_combine with key_idx (N x uint32) in place of PK; format JJS_FORMAT_AFFINE or JJS_FORMAT_EXT (R, S)
    void multisig_combine(int format, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                          const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* agg_pk,
                          uint8_t* sig_u, uint8_t* sig_R) const {
        int rc = jjs_multisig_combine_keyset(handle_, format, key_idx, z, R, S, m, offsets, n_transcripts, share_status, transcript_status, agg_pk,
                                             sig_u, sig_R);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_combine_keyset");
    }
    // raw form of verify_share against the set (jjs_multisig_verify_share_keyset): host buffers, blocking; the transcripts of
    // multisig_combine, n_shares queries (share_transcript, share_slot: uint32; z: 32 bytes each), share_status n_shares bytes,
    // sig_R nullable (n_transcripts x 64); format JJS_FORMAT_AFFINE, _EXT or _WIRE (R, S)
    void multisig_verify_share(int format, const uint32_t* key_idx, const uint8_t* R, const uint8_t* S, const uint8_t* m, const uint32_t* offsets,
                               size_t n_transcripts, const uint32_t* share_transcript, const uint32_t* share_slot, const uint8_t* z,
                               size_t n_shares, uint8_t* share_status, uint8_t* sig_R = nullptr) const {
        int rc = jjs_multisig_verify_share_keyset(handle_, format, key_idx, R, S, m, offsets, n_transcripts, share_transcript, share_slot, z, n_shares,
                                                  share_status, sig_R);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_verify_share_keyset");
    }
    // verify_share(share, participant_index, ., R_vec, S_vec, msg) of ONE transcript whose signers are keys of this set, named by
    // index in the committee's order: as multisig::verify_share (defined behind it); a transcript the engine refuses is BytesError
    inline std::optional<multisig::CombineError> multisig_verify_share(const JubJubScalar& share, size_t participant_index,
                                                                       const std::vector<uint32_t>& key_idx, const std::vector<ExtendedPoint>& R_vec,
                                                                       const std::vector<ExtendedPoint>& S_vec, const BlsScalar& msg,
                                                                       AffinePoint* sig_R = nullptr) const;
    // `combine` of ONE transcript whose signers are keys of this set (scheme single), named by index in the committee's order;
    // R and S as the Rust side holds them.  A transcript that names an index outside the set or a key whose key_status is not 0
    // is refused by the engine: BytesError with the index of its first such row (defined behind multisig::CombineResult).
    inline multisig::CombineResult multisig_combine(const std::vector<uint32_t>& key_idx, const std::vector<JubJubScalar>& z_vec,
                                                    const std::vector<ExtendedPoint>& R_vec, const std::vector<ExtendedPoint>& S_vec,
                                                    const BlsScalar& msg) const;
    // raw forms of the verifier's multisignature calls against the set (jjs_multisig_aggregate_pk_keyset,
    // jjs_multisig_verify_keyset): host buffers, blocking; key_idx (N x uint32) names the keys of every vector, vector t owning
    // rows [offsets[t], offsets[t+1]); format (of R) JJS_FORMAT_AFFINE or JJS_FORMAT_EXT; vec_status, status and tally may be null
    void multisig_aggregate_pk(const uint32_t* key_idx, const uint32_t* offsets, size_t n_vectors, uint8_t* agg_pk, uint8_t* vec_status) const {
        int rc = jjs_multisig_aggregate_pk_keyset(handle_, key_idx, offsets, n_vectors, agg_pk, vec_status);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_aggregate_pk_keyset");
    }
    void multisig_verify(int format, const uint32_t* key_idx, const uint32_t* offsets, const uint8_t* u, const uint8_t* R, const uint8_t* m,
                         size_t n_vectors, uint8_t* agg_pk, uint8_t* status, uint64_t tally[4] = nullptr) const {
        int rc = jjs_multisig_verify_keyset(handle_, format, key_idx, offsets, u, R, m, n_vectors, agg_pk, status, tally);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_verify_keyset");
    }
    // `aggregate_pk` of ONE vector of this set's keys (scheme single), named by index in the committee's order: the aggregate key,
    // or nothing for a vector that names an index outside the set or a key whose key_status is not 0
    std::optional<AffinePoint> multisig_aggregate_pk(const std::vector<uint32_t>& key_idx) const {
        const uint32_t offsets[2] = {0, (uint32_t)key_idx.size()};
        AffinePoint agg{};
        uint8_t vst = 0;
        multisig_aggregate_pk(key_idx.data(), offsets, 1, agg.data(), &vst);
        return vst ? std::nullopt : std::optional<AffinePoint>(agg);
    }
    // `aggregate_pk(&pk_vec).verify(&sig, msg)` for ONE such vector: what PublicKey::verify answers for the aggregate key; a
    // refused vector is BytesError.  agg (nullable) receives the aggregate key (zero for a refused vector).
    VerifyResult multisig_verify(const std::vector<uint32_t>& key_idx, const Signature& sig, const BlsScalar& msg, AffinePoint* agg = nullptr) const {
        const uint32_t offsets[2] = {0, (uint32_t)key_idx.size()};
        AffinePoint a{};
        uint8_t st = 0;
        multisig_verify(JJS_FORMAT_AFFINE, key_idx.data(), offsets, sig.u.data(), sig.R.data(), msg.data(), 1, a.data(), &st);
        if (agg) *agg = a;
        return from_status(st);
    }
    // (key index, signature, message): the signature type of the set's scheme
    template <typename Sig>
    struct Item { uint32_t index; Sig sig; BlsScalar message; };
    std::vector<VerifyResult> verify_batch(const std::vector<Item<Signature>>& items) const { return batch(items, JJS_SCHEME_SINGLE); }
    std::vector<VerifyResult> verify_batch(const std::vector<Item<SignatureDouble>>& items) const { return batch(items, JJS_SCHEME_DOUBLE); }
    std::vector<VerifyResult> verify_batch(const std::vector<Item<SignatureVarGen>>& items) const { return batch(items, JJS_SCHEME_VARGEN); }

  private:
    KeySet(int scheme, const detail::Soa& a, size_t n) : KeySet(scheme, JJS_FORMAT_AFFINE, a.data(), nullptr, n) {}
    KeySet(int scheme, const detail::Soa& a, const detail::Soa& b, size_t n) : KeySet(scheme, JJS_FORMAT_AFFINE, a.data(), b.data(), n) {}
    template <typename K, typename F>
    static detail::Soa column(const std::vector<K>& keys, F get) {
        detail::Soa c(keys.size(), 64);
        for (size_t i = 0; i < keys.size(); ++i) c.put(i, 0, get(keys[i]));
        return c;
    }
    template <typename Sig>
    std::vector<VerifyResult> batch(const std::vector<Item<Sig>>& items, int scheme) const {
        if (scheme != scheme_) throw std::invalid_argument("signature type does not match the key set's scheme");
        const size_t n = items.size();
        const bool dbl = scheme == JJS_SCHEME_DOUBLE;
        std::vector<uint32_t> idx(n);
        detail::Soa u(n, 32), r(n, 64), rp(dbl ? n : 0, 64), m(n, 32);
        for (size_t i = 0; i < n; ++i) {
            idx[i] = items[i].index;
            u.put(i, 0, items[i].sig.u); r.put(i, 0, items[i].sig.R); m.put(i, 0, items[i].message);
            if constexpr (std::is_same<Sig, SignatureDouble>::value) rp.put(i, 0, items[i].sig.R_prime);
        }
        std::vector<uint8_t> status(n);
        verify(JJS_FORMAT_AFFINE, idx.data(), u.data(), r.data(), dbl ? rp.data() : nullptr, m.data(), n, status.data());
        return detail::results(status);
    }
    void reset() { if (handle_) { (void)jjs_keyset_destroy(handle_); handle_ = 0; } }
    int scheme_ = 0;
    jjs_keyset handle_ = 0;
    std::vector<uint8_t> status_;
};

// Multisig signer groups (include/jjs_gpu.h jjs_msig_group_*): the ordered key vector of a committee registered once; its
// delinearisation coefficients, aggregate key and window tables stay on the device.  Move-only; the destructor destroys the
// group (calls already queued on a stream still complete).
namespace multisig {
// reference src/error.rs: what `combine` answers instead of a signature.  InvalidMultisigShare carries the participant index of
// the first failing share (derived on the host from share_status, status 4).  BytesError is the engine's own third kind, with the same
// index: the first failing share has status 3, an encoding the Rust types cannot hold (z >= r, a coordinate >= q, Z = 0, or m >= q) --
// the reference's `combine` cannot be handed such a value and has no variant for it; it is not InvalidMultisigShare.
struct CombineError {
    enum Kind { InvalidMultisigTranscript, InvalidMultisigShare, BytesError } kind;
    size_t participant_index;     // of the first failing share; 0 for InvalidMultisigTranscript
};
struct CombineResult {
    std::optional<Signature> signature;      // present exactly when `error` is not
    std::optional<CombineError> error;
    explicit operator bool() const { return signature.has_value(); }
    // the participant slot of the first failing share -- the index of Error::InvalidMultisigShare(index), src/error.rs:25, and of
    // the engine's BytesError alike; nothing for a signature and for InvalidMultisigTranscript, which names no share
    std::optional<size_t> first_failing_slot() const {
        if (!error || error->kind == CombineError::InvalidMultisigTranscript) return std::nullopt;
        return error->participant_index;
    }
};
// `combine` (reference src/multisig.rs:326-360) of ONE transcript from the types the Rust side holds -- extended points pass
// through as get_u / get_v / get_z bytes, nothing is inverted on the host -- through the blocking host form
// jjs_multisig_combine.  An empty transcript, or vectors of unequal length: InvalidMultisigTranscript, without a call.
inline CombineResult combine(const std::vector<JubJubScalar>& z_vec, const std::vector<ExtendedPoint>& pk_vec, const std::vector<ExtendedPoint>& R_vec,
                             const std::vector<ExtendedPoint>& S_vec, const BlsScalar& msg) {
    const size_t n = pk_vec.size();
    if (n == 0 || z_vec.size() != n || R_vec.size() != n || S_vec.size() != n || n > 0xFFFFFFFFull)
        return CombineResult{std::nullopt, CombineError{CombineError::InvalidMultisigTranscript, 0}};
    const uint32_t offsets[2] = {0, (uint32_t)n};
    std::vector<uint8_t> status(n);
    uint8_t tstatus = 0;
    AffinePoint agg{}, R{};
    Scalar u{};
    // (std::array rows are contiguous: a vector of them is the n x 32 / n x 96 column the call takes)
    const int rc = jjs_multisig_combine(JJS_FORMAT_EXT, z_vec[0].data(), pk_vec[0].data(), R_vec[0].data(), S_vec[0].data(), msg.data(), offsets, 1,
                                        status.data(), &tstatus, agg.data(), u.data(), R.data());
    if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_combine");
    for (size_t i = 0; i < n; ++i)
        if (status[i])
            return CombineResult{std::nullopt, CombineError{status[i] == JJS_STATUS_INVALID_SHARE ? CombineError::InvalidMultisigShare : CombineError::BytesError, i}};
    return CombineResult{Signature{u, R}, std::nullopt};
}


// The verifier's half (reference src/multisig.rs:90-92: pk = aggregate_pk(&pk_vec); pk.verify(&sig, message)), from the types
// the Rust side holds, through the blocking host forms jjs_multisig_aggregate_pk / jjs_multisig_verify.  Keys pass through as
// get_u / get_v / get_z bytes; a vector with a key the Rust types cannot hold (a coordinate >= q, Z = 0) or that is not on the
// curve is refused.
// `aggregate_pk`: the aggregate key (the identity for an empty vector), or nothing for a refused vector.
inline std::optional<AffinePoint> aggregate_pk(const std::vector<ExtendedPoint>& pk_vec) {
    if (pk_vec.size() > 0xFFFFFFFFull) throw std::invalid_argument("a key vector is indexed with 32 bits");
    const uint32_t offsets[2] = {0, (uint32_t)pk_vec.size()};
    AffinePoint agg{};
    uint8_t vst = 0;
    const int rc = jjs_multisig_aggregate_pk(JJS_FORMAT_EXT, pk_vec.empty() ? nullptr : pk_vec[0].data(), offsets, 1, agg.data(), &vst);
    if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_aggregate_pk");
    return vst ? std::nullopt : std::optional<AffinePoint>(agg);
}
// (key vector, aggregate signature, message)
struct VerifyItem {
    std::vector<ExtendedPoint> pk_vec;
    Signature sig;
    BlsScalar message;
};
// The batch form: one result per item, as PublicKey::verify_batch gives them for the aggregate keys; BytesError for a refused
// vector.  agg (nullable) receives the aggregate keys (zero for a refused vector), tally (nullable) the four status counts.
inline std::vector<VerifyResult> verify_batch(const std::vector<VerifyItem>& items, std::vector<AffinePoint>* agg = nullptr, uint64_t tally[4] = nullptr) {
    const size_t B = items.size();
    std::vector<uint32_t> offsets(B + 1, 0);
    size_t n = 0;
    for (size_t t = 0; t < B; ++t) {
        n += items[t].pk_vec.size();
        if (n > 0xFFFFFFFFull) throw std::invalid_argument("the key rows of a call are indexed with 32 bits");
        offsets[t + 1] = (uint32_t)n;
    }
    std::vector<ExtendedPoint> pk(n), R(B);
    std::vector<Scalar> u(B), m(B);
    std::vector<AffinePoint> a(B);
    std::vector<uint8_t> status(B);
    for (size_t t = 0, at = 0; t < B; ++t) {
        for (const ExtendedPoint& p : items[t].pk_vec) pk[at++] = p;
        u[t] = items[t].sig.u; m[t] = items[t].message;
        R[t].fill(0);                                            // the affine R as (u, v, 1)
        std::memcpy(R[t].data(), items[t].sig.R.data(), 64);
        R[t][64] = 1;
    }
    if (B) {
        const int rc = jjs_multisig_verify(JJS_FORMAT_EXT, n ? pk[0].data() : nullptr, offsets.data(), u[0].data(), R[0].data(), m[0].data(), B,
                                           a[0].data(), status.data(), tally);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_verify");
    } else if (tally) {
        for (int k = 0; k < 4; ++k) tally[k] = 0;
    }
    if (agg) *agg = a;
    return detail::results(status);
}
// `aggregate_pk(&pk_vec).verify(&sig, msg)` of ONE vector: Ok, or the scheme's error as PublicKey::verify answers it
inline VerifyResult verify(const std::vector<ExtendedPoint>& pk_vec, const Signature& sig, const BlsScalar& msg, AffinePoint* agg = nullptr) {
    std::vector<AffinePoint> a;
    const VerifyResult r = verify_batch({VerifyItem{pk_vec, sig, msg}}, &a)[0];
    if (agg) *agg = a[0];
    return r;
}

// ---- from wire bytes (include/jjs_gpu.h "multisignature from wire encodings") ----
// What a combiner or a verifier holds when the data first reaches it: `to_bytes` forms, decoded on the device.  An encoding that
// `from_bytes` would reject is BytesError for its share (combine), for its vector (aggregate_pk: nothing) or its item (verify).
// (These overloads are templates that only vectors of PointBytes / VerifyItemBytes instantiate: a braced `{}` argument deduces
// nothing, so calls such as combine({}, {}, {}, {}, m) keep meaning the forms above.)
template <class P>
using if_point_bytes = std::enable_if_t<std::is_same<P, PointBytes>::value>;
// `combine` of ONE transcript from PublicKey::to_bytes keys and JubJubAffine::to_bytes nonce commitments (jjs_multisig_combine_wire).
template <class P, class = if_point_bytes<P>>
inline CombineResult combine(const std::vector<JubJubScalar>& z_vec, const std::vector<P>& pk_vec, const std::vector<P>& R_vec,
                             const std::vector<P>& S_vec, const BlsScalar& msg) {
    const size_t n = pk_vec.size();
    if (n == 0 || z_vec.size() != n || R_vec.size() != n || S_vec.size() != n || n > 0xFFFFFFFFull)
        return CombineResult{std::nullopt, CombineError{CombineError::InvalidMultisigTranscript, 0}};
    const uint32_t offsets[2] = {0, (uint32_t)n};
    std::vector<uint8_t> status(n);
    uint8_t tstatus = 0;
    AffinePoint agg{}, R{};
    Scalar u{};
    const int rc = jjs_multisig_combine_wire(z_vec[0].data(), pk_vec[0].data(), R_vec[0].data(), S_vec[0].data(), msg.data(), offsets, 1,
                                             status.data(), &tstatus, agg.data(), u.data(), R.data());
    if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_combine_wire");
    for (size_t i = 0; i < n; ++i)
        if (status[i])
            return CombineResult{std::nullopt, CombineError{status[i] == JJS_STATUS_INVALID_SHARE ? CombineError::InvalidMultisigShare : CombineError::BytesError, i}};
    return CombineResult{Signature{u, R}, std::nullopt};
}
// `aggregate_pk` from PublicKey::to_bytes keys (jjs_multisig_aggregate_pk_wire): nothing for a vector with an undecodable key
template <class P, class = if_point_bytes<P>>
inline std::optional<AffinePoint> aggregate_pk(const std::vector<P>& pk_vec) {
    if (pk_vec.size() > 0xFFFFFFFFull) throw std::invalid_argument("a key vector is indexed with 32 bits");
    const uint32_t offsets[2] = {0, (uint32_t)pk_vec.size()};
    AffinePoint agg{};
    uint8_t vst = 0;
    const int rc = jjs_multisig_aggregate_pk_wire(pk_vec.empty() ? nullptr : pk_vec[0].data(), offsets, 1, agg.data(), &vst);
    if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_aggregate_pk_wire");
    return vst ? std::nullopt : std::optional<AffinePoint>(agg);
}
// (key vector, aggregate signature, message) as bytes
struct VerifyItemBytes {
    std::vector<PointBytes> pk_vec;
    SignatureBytes sig;
    BlsScalar message;
};
template <class I, class = std::enable_if_t<std::is_same<I, VerifyItemBytes>::value>>
inline std::vector<VerifyResult> verify_batch(const std::vector<I>& items, std::vector<AffinePoint>* agg = nullptr, uint64_t tally[4] = nullptr) {
    const size_t B = items.size();
    std::vector<uint32_t> offsets(B + 1, 0);
    size_t n = 0;
    for (size_t t = 0; t < B; ++t) {
        n += items[t].pk_vec.size();
        if (n > 0xFFFFFFFFull) throw std::invalid_argument("the key rows of a call are indexed with 32 bits");
        offsets[t + 1] = (uint32_t)n;
    }
    std::vector<PointBytes> pk(n);
    std::vector<SignatureBytes> sig(B);
    std::vector<Scalar> m(B);
    std::vector<AffinePoint> a(B);
    std::vector<uint8_t> status(B);
    for (size_t t = 0, at = 0; t < B; ++t) {
        for (const PointBytes& p : items[t].pk_vec) pk[at++] = p;
        sig[t] = items[t].sig; m[t] = items[t].message;
    }
    if (B) {
        const int rc = jjs_multisig_verify_wire(n ? pk[0].data() : nullptr, offsets.data(), sig[0].data(), m[0].data(), B, a[0].data(), status.data(),
                                                tally);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_verify_wire");
    } else if (tally) {
        for (int k = 0; k < 4; ++k) tally[k] = 0;
    }
    if (agg) *agg = a;
    return detail::results(status);
}
template <class P, class = if_point_bytes<P>>
inline VerifyResult verify(const std::vector<P>& pk_vec, const SignatureBytes& sig, const BlsScalar& msg, AffinePoint* agg = nullptr) {
    std::vector<AffinePoint> a;
    const VerifyResult r = verify_batch(std::vector<VerifyItemBytes>{VerifyItemBytes{pk_vec, sig, msg}}, &a)[0];
    if (agg) *agg = a[0];
    return r;
}

// ---- verify_share on its own (reference src/multisig.rs:284-309; include/jjs_gpu.h jjs_multisig_verify_share) ----
// verify_share(share, participant_index, pk_vec, R_vec, S_vec, msg): what a coordinator checks as shares arrive.  Nothing: the
// share verifies.  InvalidMultisigTranscript (decided here, without a call, as the reference decides it before any arithmetic): an
// empty transcript, vectors of unequal length, or participant_index beyond them.  InvalidMultisigShare CARRYING participant_index:
// status 4.  BytesError with the same index: status 3, an encoding the Rust types cannot hold (share >= r, a coordinate >= q,
// Z = 0, m >= q, bytes that do not decode).  sig_R (nullable) receives the transcript's aggregate commitment, what `combine` returns as R.
// One transcript per call is no faster than `combine` with filler shares (profiles/r21_msig_share.jsonl; include/jjs_gpu.h): batch
// the queries (verify_share_batch) where shares of many transcripts are at hand.
using ShareResult = std::optional<CombineError>;
namespace share_detail {
inline ShareResult share_result(uint8_t status, size_t participant_index) {
    if (status == JJS_STATUS_OK) return std::nullopt;
    if (status == JJS_STATUS_INVALID_TRANSCRIPT) return CombineError{CombineError::InvalidMultisigTranscript, 0};
    return CombineError{status == JJS_STATUS_INVALID_SHARE ? CombineError::InvalidMultisigShare : CombineError::BytesError, participant_index};
}
template <class P>
inline ShareResult verify_share(int format, const JubJubScalar& share, size_t participant_index, const std::vector<P>& pk_vec,
                                const std::vector<P>& R_vec, const std::vector<P>& S_vec, const BlsScalar& msg, AffinePoint* sig_R) {
    const size_t n = pk_vec.size();
    if (n == 0 || R_vec.size() != n || S_vec.size() != n || participant_index >= n || n > 0xFFFFFFFFull)
        return CombineError{CombineError::InvalidMultisigTranscript, 0};
    const uint32_t offsets[2] = {0, (uint32_t)n}, transcript = 0, slot = (uint32_t)participant_index;
    uint8_t status = 0;
    const int rc = jjs_multisig_verify_share(format, pk_vec[0].data(), R_vec[0].data(), S_vec[0].data(), msg.data(), offsets, 1, &transcript, &slot,
                                             share.data(), 1, &status, sig_R ? sig_R->data() : nullptr);
    if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_verify_share");
    return share_result(status, participant_index);
}
}  // namespace share_detail
inline ShareResult verify_share(const JubJubScalar& share, size_t participant_index, const std::vector<ExtendedPoint>& pk_vec,
                                const std::vector<ExtendedPoint>& R_vec, const std::vector<ExtendedPoint>& S_vec, const BlsScalar& msg,
                                AffinePoint* sig_R = nullptr) {
    return share_detail::verify_share(JJS_FORMAT_EXT, share, participant_index, pk_vec, R_vec, S_vec, msg, sig_R);
}
// ... from PublicKey::to_bytes keys and JubJubAffine::to_bytes nonce commitments
template <class P, class = if_point_bytes<P>>
inline ShareResult verify_share(const JubJubScalar& share, size_t participant_index, const std::vector<P>& pk_vec, const std::vector<P>& R_vec,
                                const std::vector<P>& S_vec, const BlsScalar& msg, AffinePoint* sig_R = nullptr) {
    return share_detail::verify_share(JJS_FORMAT_WIRE, share, participant_index, pk_vec, R_vec, S_vec, msg, sig_R);
}
// The batch form: many transcripts, many queries in any order, one call (several queries may name one transcript or one slot).
struct ShareTranscript {
    std::vector<ExtendedPoint> pk_vec, R_vec, S_vec;
    BlsScalar message;
};
struct ShareQuery {
    size_t transcript, participant_index;
    JubJubScalar share;
};
// One result per query, as verify_share gives it; a query that names no transcript is InvalidMultisigTranscript as well.  sig_R
// (nullable) receives one aggregate commitment per transcript, zero for a transcript that is empty, malformed or of unequal vectors.
inline std::vector<ShareResult> verify_share_batch(const std::vector<ShareTranscript>& transcripts, const std::vector<ShareQuery>& queries,
                                                   std::vector<AffinePoint>* sig_R = nullptr) {
    const size_t B = transcripts.size(), Q = queries.size();
    std::vector<uint32_t> offsets(B + 1, 0);
    std::vector<bool> usable(B);
    size_t n = 0;
    for (size_t t = 0; t < B; ++t) {
        const ShareTranscript& T = transcripts[t];
        usable[t] = !T.pk_vec.empty() && T.R_vec.size() == T.pk_vec.size() && T.S_vec.size() == T.pk_vec.size();
        n += usable[t] ? T.pk_vec.size() : 0;                   // an unusable transcript travels as an empty one
        if (n > 0xFFFFFFFFull) throw std::invalid_argument("the participant rows of a call are indexed with 32 bits");
        offsets[t + 1] = (uint32_t)n;
    }
    std::vector<ExtendedPoint> pk(n), R(n), S(n);
    std::vector<Scalar> m(B), z(Q);
    std::vector<uint32_t> qt(Q), qs(Q);
    std::vector<uint8_t> status(Q);
    std::vector<AffinePoint> rsa(B);
    for (size_t t = 0, at = 0; t < B; ++t) {
        m[t] = transcripts[t].message;
        if (!usable[t]) continue;
        for (size_t i = 0; i < transcripts[t].pk_vec.size(); ++i, ++at) { pk[at] = transcripts[t].pk_vec[i]; R[at] = transcripts[t].R_vec[i]; S[at] = transcripts[t].S_vec[i]; }
    }
    std::vector<ShareResult> out(Q);
    for (size_t q = 0; q < Q; ++q) {
        const bool named = queries[q].transcript < B && usable[queries[q].transcript] &&
                           queries[q].participant_index < transcripts[queries[q].transcript].pk_vec.size();
        qt[q] = named ? (uint32_t)queries[q].transcript : 0u;
        qs[q] = named ? (uint32_t)queries[q].participant_index : 0xFFFFFFFFu;     // beyond every transcript: status 5 at most
        z[q] = queries[q].share;
    }
    if (B && (Q || sig_R)) {
        const int rc = jjs_multisig_verify_share(JJS_FORMAT_EXT, n ? pk[0].data() : nullptr, n ? R[0].data() : nullptr, n ? S[0].data() : nullptr,
                                                 m[0].data(), offsets.data(), B, Q ? qt.data() : nullptr, Q ? qs.data() : nullptr,
                                                 Q ? z[0].data() : nullptr, Q, Q ? status.data() : nullptr, sig_R ? rsa[0].data() : nullptr);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_verify_share");
    }
    for (size_t q = 0; q < Q; ++q) {
        const bool named = qs[q] != 0xFFFFFFFFu && B != 0;
        out[q] = named ? share_detail::share_result(status[q], queries[q].participant_index) : ShareResult(CombineError{CombineError::InvalidMultisigTranscript, 0});
    }
    if (sig_R) *sig_R = rsa;
    return out;
}

// ---- the signer's half (reference src/multisig.rs sign_round_1 :169-184, sign_round_2 :213-257) ----
// TEST AND BENCHMARK MATERIAL, as the engine's calls behind it (include/jjs_gpu.h jjs_multisig_sign): NOT constant time, here or
// on the device -- never with production keys.  Nothing enforces the one-shot MultisigNonce of the reference (:131-141): using
// a pair (r, s) twice is the caller's error.
// The host arithmetic below (integers mod q, the curve's unified addition, k * G by double-and-add) exists for two things the C
// ABI has no host form of: the two products of sign_round_1, and sk * G for the row search of sign_round_2.  It is slow
// (a few milliseconds per product) and plain: bit-serial products, Fermat inversion.
namespace host {
struct U256 {
    uint64_t w[4];
};
inline U256 from_bytes(const uint8_t* b) { U256 x; std::memcpy(x.w, b, 32); return x; }     // little-endian hosts, as the C ABI's columns
inline const U256& modulus() {
    static const U256 q{{0xFFFFFFFF00000001ull, 0x53BDA402FFFE5BFEull, 0x3339D80809A1D805ull, 0x73EDA753299D7D48ull}};
    return q;
}
inline bool less(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
    return false;
}
inline bool equal(const U256& a, const U256& b) { return std::memcmp(a.w, b.w, 32) == 0; }
inline U256 sub_raw(const U256& a, const U256& b) {
    U256 r;
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - (uint64_t)borrow;
        r.w[i] = (uint64_t)d;
        borrow = (d >> 64) & 1;
    }
    return r;
}
inline U256 add(const U256& a, const U256& b) {              // a, b < q < 2^255: the sum fits
    U256 r;
    unsigned __int128 carry = 0;
    for (int i = 0; i < 4; ++i) {
        carry += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)carry;
        carry >>= 64;
    }
    return less(r, modulus()) ? r : sub_raw(r, modulus());
}
inline U256 sub(const U256& a, const U256& b) { return less(a, b) ? sub_raw(modulus(), sub_raw(b, a)) : sub_raw(a, b); }
inline U256 mul(const U256& a, const U256& b) {
    U256 r{{0, 0, 0, 0}};
    for (int bit = 255; bit >= 0; --bit) {
        r = add(r, r);
        if ((b.w[bit >> 6] >> (bit & 63)) & 1) r = add(r, a);
    }
    return r;
}
inline U256 small(uint64_t x) { return U256{{x, 0, 0, 0}}; }
inline U256 inverse(const U256& a) {                         // a^(q - 2)
    const U256 e = sub_raw(modulus(), small(2));
    U256 r = small(1);
    for (int bit = 255; bit >= 0; --bit) {
        r = mul(r, r);
        if ((e.w[bit >> 6] >> (bit & 63)) & 1) r = mul(r, a);
    }
    return r;
}
struct Point {
    U256 x, y, z, t;
};
inline Point add(const Point& p, const Point& q) {          // -x^2 + y^2 = 1 + d x^2 y^2, d = -(10240 / 10241): complete
    static const U256 d2 = [] { const U256 d = sub(small(0), mul(small(10240), inverse(small(10241)))); return add(d, d); }();
    const U256 a = mul(sub(p.y, p.x), sub(q.y, q.x)), b = mul(add(p.y, p.x), add(q.y, q.x)), c = mul(mul(p.t, d2), q.t);
    const U256 zz = mul(p.z, q.z), dd = add(zz, zz), e = sub(b, a), f = sub(dd, c), g = add(dd, c), h = add(b, a);
    return Point{mul(e, f), mul(g, h), mul(f, g), mul(e, h)};
}
// k * G as affine canonical bytes, G the generator of the reference (dusk_jubjub::GENERATOR_EXTENDED); k: 32 bytes little-endian
inline AffinePoint mul_generator(const Scalar& k) {
    const U256 gx{{0x4DF7B7FFEC7BEACAull, 0x2E3EBB21FD6C54EDull, 0xF1FBF02D0FD6CCE6ull, 0x3FD2814C43AC65A6ull}}, gy = small(0x12);
    const Point g{gx, gy, small(1), mul(gx, gy)};
    Point acc{small(0), small(1), small(1), small(0)};
    for (int bit = 255; bit >= 0; --bit) {
        acc = add(acc, acc);
        if ((k[bit >> 3] >> (bit & 7)) & 1) acc = add(acc, g);
    }
    const U256 zi = inverse(acc.z), u = mul(acc.x, zi), v = mul(acc.y, zi);
    AffinePoint out;
    std::memcpy(out.data(), u.w, 32);
    std::memcpy(out.data() + 32, v.w, 32);
    return out;
}
// the extended point (U, V, Z) is the affine point a: U = u Z and V = v Z with every coordinate canonical and Z != 0
inline bool same_point(const ExtendedPoint& e, const AffinePoint& a) {
    const U256 U = from_bytes(e.data()), V = from_bytes(e.data() + 32), Z = from_bytes(e.data() + 64);
    if (!less(U, modulus()) || !less(V, modulus()) || !less(Z, modulus()) || equal(Z, small(0))) return false;
    return equal(U, mul(from_bytes(a.data()), Z)) && equal(V, mul(from_bytes(a.data() + 32), Z));
}
}  // namespace host

// `sign_round_1` given the two RNG draws: (R, S) = (r * G, s * G).  Host arithmetic; no engine call.
inline std::pair<AffinePoint, AffinePoint> sign_round_1(const JubJubScalar& r, const JubJubScalar& s) {
    return {host::mul_generator(r), host::mul_generator(s)};
}
struct SignResult {
    std::optional<JubJubScalar> share;       // present exactly when `error` is not
    std::optional<Error> error;              // InvalidMultisigTranscript, DuplicatedNonce, or BytesError (status 3: an encoding the Rust types cannot hold)
    explicit operator bool() const { return share.has_value(); }
};
// `sign_round_2` of ONE transcript from the types the Rust side holds, through the blocking host form jjs_multisig_sign.  The
// engine's call is told the signer's row; the reference searches pk_vec for the signer's key, and so does this function, on the
// host: the rows of pk_vec that are the point sk * G.  None, or more than one ("occurs exactly once", :223-231), or vectors of
// unequal length, or an empty transcript: InvalidMultisigTranscript, without a call.
inline SignResult sign_round_2(const JubJubScalar& sk, const JubJubScalar& r, const JubJubScalar& s, const std::vector<ExtendedPoint>& pk_vec,
                               const std::vector<ExtendedPoint>& R_vec, const std::vector<ExtendedPoint>& S_vec, const BlsScalar& msg) {
    const size_t n = pk_vec.size();
    if (n == 0 || R_vec.size() != n || S_vec.size() != n || n > 0xFFFFFFFFull) return SignResult{std::nullopt, Error::InvalidMultisigTranscript};
    const AffinePoint mine = host::mul_generator(sk);
    size_t found = 0;
    uint32_t row = 0;
    for (size_t i = 0; i < n; ++i)
        if (host::same_point(pk_vec[i], mine)) { row = (uint32_t)i; ++found; }
    if (found != 1) return SignResult{std::nullopt, Error::InvalidMultisigTranscript};
    const uint32_t offsets[2] = {0, (uint32_t)n};
    JubJubScalar z{};
    uint8_t status = 0;
    const int rc = jjs_multisig_sign(JJS_FORMAT_EXT, pk_vec[0].data(), R_vec[0].data(), S_vec[0].data(), msg.data(), offsets, 1, &row, sk.data(),
                                     r.data(), s.data(), 1, z.data(), &status);
    if (rc != JJS_OK) throw EngineError(rc, "jjs_multisig_sign");
    switch (status) {
    case JJS_STATUS_OK: return SignResult{z, std::nullopt};
    case JJS_STATUS_INVALID_TRANSCRIPT: return SignResult{std::nullopt, Error::InvalidMultisigTranscript};
    case JJS_STATUS_DUPLICATED_NONCE: return SignResult{std::nullopt, Error::DuplicatedNonce};
    default: return SignResult{std::nullopt, Error::BytesError};
    }
}

}  // namespace multisig

inline multisig::CombineResult KeySet::multisig_combine(const std::vector<uint32_t>& key_idx, const std::vector<JubJubScalar>& z_vec,
                                                        const std::vector<ExtendedPoint>& R_vec, const std::vector<ExtendedPoint>& S_vec,
                                                        const BlsScalar& msg) const {
    using namespace multisig;
    const size_t n = key_idx.size();
    if (n == 0 || z_vec.size() != n || R_vec.size() != n || S_vec.size() != n || n > 0xFFFFFFFFull)
        return CombineResult{std::nullopt, CombineError{CombineError::InvalidMultisigTranscript, 0}};
    const uint32_t offsets[2] = {0, (uint32_t)n};
    std::vector<uint8_t> status(n);
    uint8_t tstatus = 0;
    AffinePoint agg{}, R{};
    Scalar u{};
    multisig_combine(JJS_FORMAT_EXT, key_idx.data(), z_vec[0].data(), R_vec[0].data(), S_vec[0].data(), msg.data(), offsets, 1, status.data(), &tstatus,
                     agg.data(), u.data(), R.data());
    if (tstatus)
        for (size_t i = 0; i < n; ++i)           // a refused transcript: its first unusable row, from the indices and the set's key_status
            if (key_idx[i] >= status_.size() || status_[key_idx[i]] != 0) return CombineResult{std::nullopt, CombineError{CombineError::BytesError, i}};
    for (size_t i = 0; i < n; ++i)
        if (status[i])
            return CombineResult{std::nullopt, CombineError{status[i] == JJS_STATUS_INVALID_SHARE ? CombineError::InvalidMultisigShare : CombineError::BytesError, i}};
    return CombineResult{Signature{u, R}, std::nullopt};
}

inline std::optional<multisig::CombineError> KeySet::multisig_verify_share(const JubJubScalar& share, size_t participant_index,
                                                                           const std::vector<uint32_t>& key_idx,
                                                                           const std::vector<ExtendedPoint>& R_vec,
                                                                           const std::vector<ExtendedPoint>& S_vec, const BlsScalar& msg,
                                                                           AffinePoint* sig_R) const {
    using namespace multisig;
    const size_t n = key_idx.size();
    if (n == 0 || R_vec.size() != n || S_vec.size() != n || participant_index >= n || n > 0xFFFFFFFFull)
        return CombineError{CombineError::InvalidMultisigTranscript, 0};
    const uint32_t offsets[2] = {0, (uint32_t)n}, transcript = 0, slot = (uint32_t)participant_index;
    uint8_t status = 0;
    multisig_verify_share(JJS_FORMAT_EXT, key_idx.data(), R_vec[0].data(), S_vec[0].data(), msg.data(), offsets, 1, &transcript, &slot, share.data(), 1,
                          &status, sig_R ? sig_R->data() : nullptr);
    return share_detail::share_result(status, participant_index);
}

namespace multisig {
class SignerGroup {
  public:
    // PK: host, n x 64 affine, the ordered pk_vec
    SignerGroup(const uint8_t* PK, size_t n) : participants_(n) {
        int rc = jjs_msig_group_create(PK, n, &handle_);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_create");
        rc = jjs_msig_group_aggregate_pk(handle_, aggregate_pk_.data());
        if (rc != JJS_OK) { reset(); throw EngineError(rc, "jjs_msig_group_aggregate_pk"); }
    }
    explicit SignerGroup(const std::vector<AffinePoint>& keys) : SignerGroup(flat(keys).data(), keys.size()) {}
    // the ordered pk_vec as the Rust side holds it (jjs_msig_group_create_ext): the same group as from the affine forms
    explicit SignerGroup(const std::vector<ExtendedPoint>& keys) : participants_(keys.size()) {
        int rc = jjs_msig_group_create_ext(keys.empty() ? nullptr : keys[0].data(), keys.size(), &handle_);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_create_ext");
        rc = jjs_msig_group_aggregate_pk(handle_, aggregate_pk_.data());
        if (rc != JJS_OK) { reset(); throw EngineError(rc, "jjs_msig_group_aggregate_pk"); }
    }
    // ... and as PublicKey::to_bytes (jjs_msig_group_create_wire): the group of the keys they decode to
    explicit SignerGroup(const std::vector<PointBytes>& keys) : participants_(keys.size()) {
        int rc = jjs_msig_group_create_wire(keys.empty() ? nullptr : keys[0].data(), keys.size(), &handle_);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_create_wire");
        rc = jjs_msig_group_aggregate_pk(handle_, aggregate_pk_.data());
        if (rc != JJS_OK) { reset(); throw EngineError(rc, "jjs_msig_group_aggregate_pk"); }
    }
    SignerGroup(SignerGroup&& o) noexcept : handle_(o.handle_), participants_(o.participants_), aggregate_pk_(o.aggregate_pk_) { o.handle_ = 0; }
    SignerGroup& operator=(SignerGroup&& o) noexcept {
        if (this != &o) { reset(); handle_ = o.handle_; participants_ = o.participants_; aggregate_pk_ = o.aggregate_pk_; o.handle_ = 0; }
        return *this;
    }
    SignerGroup(const SignerGroup&) = delete;
    SignerGroup& operator=(const SignerGroup&) = delete;
    ~SignerGroup() { reset(); }

    jjs_msig_group handle() const { return handle_; }
    size_t participants() const { return participants_; }
    // aggregate_pk(pk_vec), 64 bytes affine
    const AffinePoint& aggregate_pk() const { return aggregate_pk_; }
    std::array<uint64_t, JJS_MSIG_GROUP_INFO> info() const {
        std::array<uint64_t, JJS_MSIG_GROUP_INFO> out{};
        int rc = jjs_msig_group_info(handle_, out.data());
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_info");
        return out;
    }
    // device pointers (16-byte aligned), asynchronous on `stream` (a hipStream_t): the columns and outputs of
    // jjs_msig_group_combine_dev for n_transcripts transcripts of participants() shares each
    void combine_dev(const void* z, const void* R, const void* S, const void* m, size_t n_transcripts, void* share_status,
                     void* transcript_status, void* sig_u, void* sig_R, void* stream = nullptr) const {
        int rc = jjs_msig_group_combine_dev(handle_, z, R, S, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, stream);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_combine_dev");
    }
    // the same with R and S as B n x 96 extended points (jjs_msig_group_combine_ext_dev)
    void combine_ext_dev(const void* z, const void* R_ext, const void* S_ext, const void* m, size_t n_transcripts, void* share_status,
                         void* transcript_status, void* sig_u, void* sig_R, void* stream = nullptr) const {
        int rc = jjs_msig_group_combine_ext_dev(handle_, z, R_ext, S_ext, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, stream);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_combine_ext_dev");
    }
    // the same with R and S as B n x 32 wire encodings (jjs_msig_group_combine_wire_dev), and from host buffers, blocking
    void combine_wire_dev(const void* z, const void* R_w, const void* S_w, const void* m, size_t n_transcripts, void* share_status,
                          void* transcript_status, void* sig_u, void* sig_R, void* stream = nullptr) const {
        int rc = jjs_msig_group_combine_wire_dev(handle_, z, R_w, S_w, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, stream);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_combine_wire_dev");
    }
    void combine_wire(const uint8_t* z, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m, size_t n_transcripts, uint8_t* share_status,
                      uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) const {
        int rc = jjs_msig_group_combine_wire(handle_, z, R_w, S_w, m, n_transcripts, share_status, transcript_status, sig_u, sig_R);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_combine_wire");
    }
    // host buffers, blocking (jjs_msig_group_combine): format JJS_FORMAT_AFFINE (R, S: B n x 64) or JJS_FORMAT_EXT (B n x 96)
    void combine(int format, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m, size_t n_transcripts, uint8_t* share_status,
                 uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) const {
        int rc = jjs_msig_group_combine(handle_, format, z, R, S, m, n_transcripts, share_status, transcript_status, sig_u, sig_R);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_combine");
    }
    // verify_share against the group, raw forms (jjs_msig_group_verify_share[_dev]): the transcripts of `combine`, n_shares queries
    // (share_transcript, share_slot: uint32; z: 32 bytes each), share_status n_shares bytes, sig_R nullable (n_transcripts x 64);
    // format JJS_FORMAT_AFFINE, _EXT or _WIRE (R, S)
    void verify_share(int format, const uint8_t* R, const uint8_t* S, const uint8_t* m, size_t n_transcripts, const uint32_t* share_transcript,
                      const uint32_t* share_slot, const uint8_t* z, size_t n_shares, uint8_t* share_status, uint8_t* sig_R = nullptr) const {
        int rc = jjs_msig_group_verify_share(handle_, format, R, S, m, n_transcripts, share_transcript, share_slot, z, n_shares, share_status, sig_R);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_verify_share");
    }
    void verify_share_dev(int format, const void* R, const void* S, const void* m, size_t n_transcripts, const void* share_transcript,
                          const void* share_slot, const void* z, size_t n_shares, void* share_status, void* sig_R = nullptr,
                          void* stream = nullptr) const {
        int rc = jjs_msig_group_verify_share_dev(handle_, format, R, S, m, n_transcripts, share_transcript, share_slot, z, n_shares, share_status,
                                                 sig_R, stream);
        if (rc != JJS_OK) throw EngineError(rc, "jjs_msig_group_verify_share_dev");
    }
    // verify_share(share, participant_index, ., R_vec, S_vec, msg) of ONE transcript of the group's signers, as multisig::verify_share
    ShareResult verify_share(const JubJubScalar& share, size_t participant_index, const std::vector<ExtendedPoint>& R_vec,
                             const std::vector<ExtendedPoint>& S_vec, const BlsScalar& msg, AffinePoint* sig_R = nullptr) const {
        if (R_vec.size() != participants_ || S_vec.size() != participants_ || participant_index >= participants_)
            return CombineError{CombineError::InvalidMultisigTranscript, 0};
        const uint32_t transcript = 0, slot = (uint32_t)participant_index;
        uint8_t status = 0;
        verify_share(JJS_FORMAT_EXT, R_vec[0].data(), S_vec[0].data(), msg.data(), 1, &transcript, &slot, share.data(), 1, &status,
                     sig_R ? sig_R->data() : nullptr);
        return share_detail::share_result(status, participant_index);
    }

  private:
    static std::vector<uint8_t> flat(const std::vector<AffinePoint>& keys) {
        std::vector<uint8_t> out(keys.size() * 64);
        for (size_t i = 0; i < keys.size(); ++i) std::memcpy(out.data() + 64 * i, keys[i].data(), 64);
        return out;
    }
    void reset() { if (handle_) { (void)jjs_msig_group_destroy(handle_); handle_ = 0; } }
    jjs_msig_group handle_ = 0;
    size_t participants_ = 0;
    AffinePoint aggregate_pk_{};
};
}  // namespace multisig

// ---- Poseidon digests (include/jjs_gpu.h jjs_digest) ----
// `dusk_poseidon::Hash::digest(Domain::Other, &payload)[0]` and `Hash::digest_truncated(Domain::Other, &payload)[0]` over the
// header's BlsScalar: how a caller who holds payloads makes the `message` of every verify and sign call above.  Blocking host-buffer
// calls.  An empty payload is refused (EngineError: the engine defines no digest of no elements); a scalar >= q -- bytes
// `BlsScalar::from_bytes` refuses -- gives nullopt.
namespace poseidon {
// one digest per payload, in one call; nullopt for a payload with a non-canonical scalar
inline std::vector<std::optional<BlsScalar>> digest_batch(const std::vector<std::vector<BlsScalar>>& payloads, bool truncated = false) {
    const size_t n = payloads.size();
    std::vector<uint32_t> offsets(n + 1, 0);
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        total += payloads[i].size();
        if (total > 0xffffffffull) throw std::length_error("jjs::poseidon::digest_batch: more than 2^32 - 1 scalars");
        offsets[i + 1] = static_cast<uint32_t>(total);
    }
    detail::Soa in(total, 32), out(n, 32);
    for (size_t i = 0, e = 0; i < n; ++i)
        for (const BlsScalar& x : payloads[i]) in.put(e++, 0, x);
    std::vector<uint8_t> status(n);
    const int rc = jjs_digest(JJS_DIGEST_CANONICAL, truncated ? JJS_DIGEST_TRUNCATED : 0, in.data(), offsets.data(), 0, n, out.data(), status.data());
    if (rc != JJS_OK) throw EngineError(rc, "jjs_digest");
    std::vector<std::optional<BlsScalar>> digests(n);
    for (size_t i = 0; i < n; ++i) {
        if (status[i] != JJS_STATUS_OK) continue;
        BlsScalar d;
        std::memcpy(d.data(), out.data() + 32 * i, 32);
        digests[i] = d;
    }
    return digests;
}
inline std::optional<BlsScalar> digest(const std::vector<BlsScalar>& payload) { return digest_batch({payload}, false)[0]; }
// the low 250 bits: a JubJubScalar
inline std::optional<JubJubScalar> digest_truncated(const std::vector<BlsScalar>& payload) { return digest_batch({payload}, true)[0]; }
}  // namespace poseidon

}  // namespace jjs

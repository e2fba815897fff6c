// pvw.hpp -- header-only C++ mirror of the reference's `pvw::{params, crs, keys, crypto}`
// interface over the C ABI (include/pvw_hip.h).
//
// The reference is a Rust crate; no Rust toolchain exists in the build image, so the host
// side above the C ABI is written in C++ with the same names, argument meaning and error
// behaviour (citations are file:line under the reference checkout).  Everything heavy runs
// in libpvw_hip.so on the GPU; this header only owns handles and flat buffers.
//   polynomial  = std::vector<uint64_t> of L*l residues, limb-major (parameters.rs:433-458)
//   randomness  = a 32-byte seed (the reference uses thread_rng(), encryption.rs:138,164,180)
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pvw_hip.h"

namespace pvw_host {

using Seed = std::array<uint8_t, 32>;

// PvwError (src/errors.rs:13-70)
class PvwError : public std::runtime_error {
 public:
  int32_t code;
  PvwError(int32_t c, const std::string& m) : std::runtime_error(variant_name(c) + ": " + m), code(c) {}
  static std::string variant_name(int32_t c) {
    static const char* names[] = {"Ok", "InvalidParameters", "SamplingError", "EncryptionError", "DecryptionError",
                                  "KeyGenerationError", "CrsError", "SerializationError", "DeserializationError",
                                  "EncodingError", "DecodingError", "ValidationError", "ContextError",
                                  "PolynomialError", "MatrixError", "DimensionMismatch", "IndexOutOfBounds",
                                  "InsufficientData", "InvalidFormat", "InternalError"};
    return (c >= 0 && c <= 19) ? names[c] : "Unknown";
  }
  std::string variant() const { return variant_name(code); }
};
inline void check(int32_t rc) {
  if (rc == PVW_OK) return;
  char buf[512];
  pvw_last_error(buf, sizeof buf);
  throw PvwError(rc, buf);
}

// PvwParameters (src/params/parameters.rs:19-40) + the device context behind it
class PvwParameters {
 public:
  uint32_t n, k, l, t;
  std::vector<uint64_t> moduli_;
  float secret_variance;
  uint64_t error_bound_1, error_bound_2;
  pvw_ctx* ctx = nullptr;

  ~PvwParameters() { pvw_ctx_destroy(ctx); }
  PvwParameters(const PvwParameters&) = delete;
  PvwParameters& operator=(const PvwParameters&) = delete;
  PvwParameters() = default;

  size_t L() const { return moduli_.size(); }
  size_t poly_words() const { return L() * l; }
  const std::vector<uint64_t>& moduli() const { return moduli_; }                    // :389
  bool verify_correctness_condition() const {                                        // :510-551
    int32_t ok = 0;
    check(pvw_ctx_verify_correctness_condition(ctx, &ok));
    return ok != 0;
  }
  std::vector<uint64_t> delta() const { return big(pvw_ctx_delta); }                  // :370 (LE 64-bit words)
  std::vector<uint64_t> q_total() const { return big(pvw_ctx_q_total); }              // :380
  std::vector<uint64_t> gadget_polynomial(uint32_t repr = PVW_REPR_POWER) const {     // :288-308
    std::vector<uint64_t> g(poly_words());
    check(pvw_ctx_gadget(ctx, g.data(), repr));
    return g;
  }
  std::vector<uint64_t> encode_scalar(int64_t scalar, uint32_t repr = PVW_REPR_POWER) const {   // :346-367
    std::vector<uint64_t> g(poly_words());
    check(pvw_encode_scalar(ctx, scalar, g.data(), repr));
    return g;
  }
  static std::pair<uint32_t, uint32_t> suggest_error_bounds(uint32_t n, uint32_t k, uint32_t l,
                                                            const std::vector<uint64_t>& moduli, float variance) {  // :554-603
    uint32_t b1 = 0, b2 = 0;
    check(pvw_suggest_error_bounds(n, k, l, moduli.data(), (uint32_t)moduli.size(), variance, &b1, &b2));
    return {b1, b2};
  }

 private:
  template <class F>
  std::vector<uint64_t> big(F fn) const {
    size_t nw = 0;
    check(fn(ctx, nullptr, 0, &nw));
    std::vector<uint64_t> w(nw);
    check(fn(ctx, w.data(), w.size(), &nw));
    return w;
  }
};

// PvwParametersBuilder (parameters.rs:44-201)
class PvwParametersBuilder {
  std::optional<uint32_t> n_, k_, l_;
  std::optional<std::vector<uint64_t>> moduli_;
  std::optional<float> variance_;
  std::optional<uint64_t> b1_, b2_;
  int32_t device_ = -1;
  uint32_t shard_[4] = {0, 0, 0, 0};

 public:
  PvwParametersBuilder& set_parties(uint32_t n) { n_ = n; return *this; }
  PvwParametersBuilder& set_dimension(uint32_t k) { k_ = k; return *this; }
  PvwParametersBuilder& set_l(uint32_t l) { l_ = l; return *this; }
  PvwParametersBuilder& set_moduli(const std::vector<uint64_t>& m) { moduli_ = m; return *this; }
  PvwParametersBuilder& set_secret_variance(float v) { variance_ = v; return *this; }
  PvwParametersBuilder& set_error_bound_1(uint64_t b) { b1_ = b; return *this; }
  PvwParametersBuilder& set_error_bound_2(uint64_t b) { b2_ = b; return *this; }
  PvwParametersBuilder& set_error_bounds_u32(uint32_t a, uint32_t b) { b1_ = a; b2_ = b; return *this; }
  PvwParametersBuilder& set_device(int32_t d) { device_ = d; return *this; }
  PvwParametersBuilder& set_shard(uint32_t plo, uint32_t phi, uint32_t clo, uint32_t chi) {
    shard_[0] = plo; shard_[1] = phi; shard_[2] = clo; shard_[3] = chi;
    return *this;
  }
  std::shared_ptr<PvwParameters> build_arc() const {                                  // :117-201
    if (!n_) throw PvwError(1, "n not set");
    if (!k_) throw PvwError(1, "k not set");
    if (!l_) throw PvwError(1, "l not set");
    if (!moduli_) throw PvwError(1, "moduli not set");
    auto p = std::make_shared<PvwParameters>();
    p->n = *n_; p->k = *k_; p->l = *l_; p->moduli_ = *moduli_;
    p->secret_variance = variance_.value_or(0.5f);                                    // :166
    p->error_bound_1 = b1_.value_or(100);                                             // :167
    p->error_bound_2 = b2_.value_or(200);                                             // :168
    p->t = *n_ ? (*n_ - 1) / 2 : 0;                                                   // :169
    pvw_params_t c{};
    c.n = p->n; c.k = p->k; c.l = p->l; c.num_moduli = (uint32_t)p->moduli_.size(); c.moduli = p->moduli_.data();
    c.secret_variance = p->secret_variance; c.error_bound_1 = p->error_bound_1; c.error_bound_2 = p->error_bound_2;
    c.device = device_; c.party_lo = shard_[0]; c.party_hi = shard_[1]; c.c1_lo = shard_[2]; c.c1_hi = shard_[3];
    check(pvw_ctx_create(&c, &p->ctx));
    return p;
  }
};

// PvwCrs (src/params/crs.rs:12-17): the k x k matrix is resident on the device of `params`
class PvwCrs {
 public:
  std::shared_ptr<PvwParameters> params;
  static PvwCrs new_deterministic(const std::shared_ptr<PvwParameters>& p, const Seed& seed) {   // crs.rs:45-67
    check(pvw_crs_generate(p->ctx, seed.data()));
    return PvwCrs{p};
  }
  // PvwCrs::new (crs.rs:24-39): a fresh random CRS; `rng` is any callable returning random 32-bit words
  // (default: std::random_device, the OS entropy source -- the reference takes a CryptoRng)
  template <class Rng>
  static PvwCrs create(const std::shared_ptr<PvwParameters>& p, Rng& rng) {
    Seed seed;
    for (size_t i = 0; i < 32; i += 4) {
      const uint32_t w = (uint32_t)rng();
      for (size_t b = 0; b < 4; ++b) seed[i + b] = (uint8_t)(w >> (8 * b));
    }
    return new_deterministic(p, seed);
  }
  static PvwCrs create(const std::shared_ptr<PvwParameters>& p) {
    std::random_device rd;
    return create(p, rd);
  }
  // PvwCrs::new_from_tag (crs.rs:74-90): the seed is DefaultHasher(tag + "CRS"), 8 LE bytes repeated four times
  static Seed seed_from_tag(const std::string& tag) {
    Seed seed;
    check(pvw_crs_seed_from_tag(tag.c_str(), seed.data()));
    return seed;
  }
  static PvwCrs new_from_tag(const std::shared_ptr<PvwParameters>& p, const std::string& tag) {
    return new_deterministic(p, seed_from_tag(tag));
  }
  static PvwCrs from_polynomials(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& a,
                                 uint32_t repr = PVW_REPR_POWER) {
    if (a.size() != (size_t)p->k * p->k * p->poly_words()) throw PvwError(15, "CRS size mismatch");
    check(pvw_load_crs(p->ctx, a.data(), repr));
    return PvwCrs{p};
  }
  std::pair<uint32_t, uint32_t> dimensions() const { return {params->k, params->k}; }
};

// SecretKey (src/keys/secret_key.rs:14-18): k x l CBD coefficients
class SecretKey {
 public:
  std::shared_ptr<PvwParameters> params;
  std::vector<int64_t> secret_coeffs;   // [k][l]
  SecretKey(std::shared_ptr<PvwParameters> p, std::vector<int64_t> c) : params(std::move(p)), secret_coeffs(std::move(c)) {}
  SecretKey(const SecretKey&) = default;
  SecretKey(SecretKey&&) = default;
  // assignment wipes what the key held before the vector lets go of it (Zeroize, secret_key.rs:20-30)
  SecretKey& operator=(const SecretKey& o) {
    if (this != &o) { zeroize(); params = o.params; secret_coeffs = o.secret_coeffs; }
    return *this;
  }
  SecretKey& operator=(SecretKey&& o) noexcept {
    if (this != &o) { zeroize(); params = std::move(o.params); secret_coeffs = std::move(o.secret_coeffs); }
    return *this;
  }
  ~SecretKey() { zeroize(); }                                   // ZeroizeOnDrop (secret_key.rs:20-30)
  static SecretKey random(const std::shared_ptr<PvwParameters>& p, const Seed& seed, uint32_t party_index) {   // :45-63
    SecretKey s{p, std::vector<int64_t>((size_t)p->k * p->l)};
    check(pvw_sample_secret_keys(p->ctx, seed.data(), party_index, 1, s.secret_coeffs.data()));
    return s;
  }
  // Zeroize: the coefficients are overwritten through a volatile pointer (not elided as a dead store); the device
  // side clears its own copies before every key-bearing call returns (pvw_selftest_secret_residue)
  void zeroize() {
    volatile int64_t* p = secret_coeffs.data();
    for (size_t i = 0; i < secret_coeffs.size(); ++i) p[i] = 0;
  }
  size_t len() const { return params->k; }
};

// A SecretKey kept on the device in the form the inner products of decrypt read (pvw_sk_load: NTT(sk[j]),
// secret_key.rs:98-112) for pvw_decrypt_batch_device_sk; cleared when the handle goes (pvw_sk_free), as the reference's
// SecretKey is ZeroizeOnDrop (secret_key.rs:20-30).  Keeps its parameters alive.
class DeviceSecretKey {
 public:
  explicit DeviceSecretKey(const SecretKey& sk) : params_(sk.params) { check(pvw_sk_load(params_->ctx, sk.secret_coeffs.data(), &key_)); }
  // the resident key of SecretKey::random(p, seed, party_index), drawn on the device (pvw_sk_load_seeded): no coefficients
  // on the host or in a device buffer
  DeviceSecretKey(const std::shared_ptr<PvwParameters>& p, const Seed& seed, uint32_t party_index) : params_(p) {
    check(pvw_sk_load_seeded(params_->ctx, seed.data(), party_index, &key_));
  }
  DeviceSecretKey(const DeviceSecretKey&) = delete;
  DeviceSecretKey& operator=(const DeviceSecretKey&) = delete;
  DeviceSecretKey(DeviceSecretKey&& o) noexcept : params_(std::move(o.params_)), key_(o.key_) { o.key_ = nullptr; }
  ~DeviceSecretKey() { if (key_) pvw_sk_free(key_); }
  const pvw_sk* raw() const { return key_; }

 private:
  std::shared_ptr<PvwParameters> params_;
  pvw_sk* key_ = nullptr;
};

// A randomness state on the device (pvw_rnd_state): seed S and counter c.  Encrypts that take it draw call_seed(S, c + i)
// when their kernels run and advance c themselves, so captured / queued calls get fresh randomness each time -- what the
// reference's thread_rng() gives every encrypt (encryption.rs:135-167).  Seeded once from the OS by default.  Ordered by
// the stream of the calls that use it; cleared and freed when the handle goes.  Keeps its parameters alive.
class DeviceRandomness {
 public:
  DeviceRandomness(const std::shared_ptr<PvwParameters>& p, const Seed& seed, uint64_t counter = 0) : params_(p) {
    check(pvw_rnd_state_create(params_->ctx, seed.data(), counter, &st_));
  }
  explicit DeviceRandomness(const std::shared_ptr<PvwParameters>& p) : DeviceRandomness(p, os_seed()) {}
  DeviceRandomness(const DeviceRandomness&) = delete;
  DeviceRandomness& operator=(const DeviceRandomness&) = delete;
  DeviceRandomness(DeviceRandomness&& o) noexcept : params_(std::move(o.params_)), st_(o.st_) { o.st_ = nullptr; }
  ~DeviceRandomness() { if (st_) pvw_rnd_state_free(st_); }
  // the counter once the work enqueued on `stream` (NULL: the context's stream) is done
  uint64_t counter(void* stream = nullptr) const { uint64_t v = 0; check(pvw_rnd_state_counter(st_, stream, &v)); return v; }
  void set_counter(uint64_t c, void* stream = nullptr) { check(pvw_rnd_state_set_counter(st_, c, stream)); }
  // the seed a call that runs at counter c draws from (host only)
  static Seed call_seed(const Seed& seed, uint64_t c) { Seed out{}; check(pvw_rnd_call_seed(seed.data(), c, out.data())); return out; }
  void* raw() const { return st_; }
  const std::shared_ptr<PvwParameters>& params() const { return params_; }

 private:
  static Seed os_seed() {
    std::random_device rd;
    Seed s{};
    for (size_t i = 0; i < s.size(); i += 4) {
      const uint32_t w = rd();
      for (size_t b = 0; b < 4; ++b) s[i + b] = (uint8_t)(w >> (8 * b));
    }
    return s;
  }
  std::shared_ptr<PvwParameters> params_;
  void* st_ = nullptr;  // pvw_rnd_state handle
};

// Party (src/keys/public_key.rs:17-22)
class Party {
 public:
  uint32_t index;
  SecretKey secret_key;
  static Party create(uint32_t index, const std::shared_ptr<PvwParameters>& p, const Seed& seed) {   // Party::new :62-79
    if (index >= p->n)
      throw PvwError(1, "Party index " + std::to_string(index) + " exceeds maximum " + std::to_string(p->n - 1));
    return Party{index, SecretKey::random(p, seed, index)};
  }
};

// SecretKey::random for parties [party_lo, party_lo + count) straight into caller-owned device memory [count][k][l] on the
// caller's stream (pvw_sample_secret_keys_device): the d_sk of the *_device decrypt calls.  The caller clears the buffer.
inline void sample_secret_keys_device(const std::shared_ptr<PvwParameters>& p, const Seed& seed, uint32_t party_lo, uint32_t count,
                                      int64_t* d_sk_out, void* stream = nullptr) {
  check(pvw_sample_secret_keys_device(p->ctx, seed.data(), party_lo, count, d_sk_out, stream));
}

// GlobalPublicKey (public_key.rs:43-54): the n x k matrix B is resident on the device
class GlobalPublicKey {
 public:
  PvwCrs crs;
  std::shared_ptr<PvwParameters> params;
  explicit GlobalPublicKey(const PvwCrs& c) : crs(c), params(c.params) {}
  void add_public_key(uint32_t index, const std::vector<uint64_t>& key_polynomials, uint32_t repr = PVW_REPR_POWER) {   // :214-250
    if (key_polynomials.size() != (size_t)params->k * params->poly_words()) throw PvwError(1, "Public key dimension mismatch");
    check(pvw_load_pk(params->ctx, index, index + 1, key_polynomials.data(), repr));
  }
  void generate_and_add_party(const Party& party, const Seed& seed) {                                  // :256-263
    check(pvw_keygen(params->ctx, party.index, party.index + 1, party.secret_key.secret_coeffs.data(), nullptr, seed.data()));
  }
  void generate_all_party_keys(const std::vector<Party>& parties, const Seed& seed) {                  // :376-401
    if (parties.size() > params->n) throw PvwError(1, "Too many parties");
    // every run of consecutive party indices is ONE batched device call (the reference generates in parallel and
    // adds in order, :387-399)
    for (size_t i = 0; i < parties.size();) {
      size_t j = i + 1;
      while (j < parties.size() && parties[j].index == parties[j - 1].index + 1) ++j;
      std::vector<int64_t> sk;
      for (size_t x = i; x < j; ++x) sk.insert(sk.end(), parties[x].secret_key.secret_coeffs.begin(), parties[x].secret_key.secret_coeffs.end());
      const int32_t rc = pvw_keygen(params->ctx, parties[i].index, parties[i].index + (uint32_t)(j - i), sk.data(), nullptr, seed.data());
      volatile int64_t* w = sk.data();
      for (size_t x = 0; x < sk.size(); ++x) w[x] = 0;
      check(rc);
      i = j;
    }
  }
  // generate_all_party_keys over Party::new (:376-401, :62-79) with the secret keys drawn on the device from sk_seed
  // (pvw_keygen_seeded): party p's key is SecretKey::random(params, sk_seed, p); it never exists on the host
  void generate_all_party_keys(uint32_t party_lo, uint32_t party_hi, const Seed& sk_seed, const Seed& seed) {
    check(pvw_keygen_seeded(params->ctx, party_lo, party_hi, sk_seed.data(), seed.data()));
  }
  uint32_t num_public_keys() const { uint32_t v = 0; check(pvw_num_public_keys(params->ctx, &v)); return v; }   // :344
  bool is_full() const { int32_t v = 0; check(pvw_is_full(params->ctx, &v)); return v != 0; }                   // :349
  std::pair<uint32_t, uint32_t> dimensions() const { return {params->n, params->k}; }
  // wire format v1: rows [lo, hi) as a kind-3 blob, packed on the device
  std::vector<uint8_t> to_bytes(uint32_t lo, uint32_t hi, uint32_t repr = PVW_REPR_POWER) const {
    size_t hl = 0, pb = 0;
    check(pvw_wire_header(params->ctx, 3, repr, lo, hi, 0, 0, nullptr, 0, &hl));
    check(pvw_wire_poly_bytes(params->ctx, &pb));
    std::vector<uint8_t> out(hl + (size_t)(hi - lo) * params->k * pb);
    check(pvw_wire_header(params->ctx, 3, repr, lo, hi, 0, 0, out.data(), hl, &hl));
    check(pvw_get_pk_wire(params->ctx, lo, hi, out.data() + hl, repr));
    return out;
  }
  // the rows of a kind-3 blob, checked before anything is stored (DeserializationError leaves the key as it was)
  void load_bytes(const std::vector<uint8_t>& blob) {
    uint32_t kind = 0, repr = 0, r[4] = {0, 0, 0, 0};
    size_t hl = 0;
    check(pvw_wire_header_check(params->ctx, blob.data(), blob.size(), &kind, &repr, r, &hl));
    if (kind != 3) throw PvwError(PVW_ERR_INVALID_FORMAT, "wire: not a public-key blob");
    check(pvw_load_pk_wire(params->ctx, r[0], r[1], blob.data() + hl, repr));
  }
  static GlobalPublicKey from_bytes(const PvwCrs& crs, const std::vector<uint8_t>& blob) {
    GlobalPublicKey g(crs);
    g.load_bytes(blob);
    return g;
  }
};

// PvwCiphertext (src/crypto/encryption.rs:15-24)
class PvwCiphertext {
 public:
  std::vector<uint64_t> c1, c2;   // [k][L][l], [n][L][l]
  std::shared_ptr<PvwParameters> params;
  uint32_t repr;
  size_t len() const { return c2.size() / params->poly_words(); }
  void validate() const {                                                                            // :41-76
    if (c1.size() != (size_t)params->k * params->poly_words()) throw PvwError(1, "c1 has the wrong number of components");
    if (c2.size() != (size_t)params->n * params->poly_words()) throw PvwError(1, "c2 has the wrong number of components");
  }
  // wire format v1: c1 rows [0, k) and c2 rows [lo, hi) as a kind-4 blob, packed on the device
  std::vector<uint8_t> to_bytes(uint32_t lo, uint32_t hi) const {
    validate();
    const size_t P = params->poly_words();
    size_t hl = 0, pb = 0;
    check(pvw_wire_header(params->ctx, 4, repr, 0, params->k, lo, hi, nullptr, 0, &hl));
    check(pvw_wire_poly_bytes(params->ctx, &pb));
    std::vector<uint64_t> polys(c1);
    polys.insert(polys.end(), c2.begin() + (size_t)lo * P, c2.begin() + (size_t)hi * P);
    const size_t count = polys.size() / P;
    std::vector<uint8_t> out(hl + count * pb);
    check(pvw_wire_header(params->ctx, 4, repr, 0, params->k, lo, hi, out.data(), hl, &hl));
    check(pvw_wire_pack(params->ctx, polys.data(), count, out.data() + hl));
    return out;
  }
  std::vector<uint8_t> to_bytes() const { return to_bytes(0, params->n); }
  // a kind-4 blob, unpacked and checked on the device; rows the blob does not carry are zero
  static PvwCiphertext from_bytes(const std::shared_ptr<PvwParameters>& p, const std::vector<uint8_t>& blob) {
    uint32_t kind = 0, rp = 0, r[4] = {0, 0, 0, 0};
    size_t hl = 0;
    check(pvw_wire_header_check(p->ctx, blob.data(), blob.size(), &kind, &rp, r, &hl));
    if (kind != 4) throw PvwError(PVW_ERR_INVALID_FORMAT, "wire: not a ciphertext blob");
    const size_t P = p->poly_words(), n1 = r[1] - r[0], n2 = r[3] - r[2];
    std::vector<uint64_t> words((n1 + n2) * P);
    check(pvw_wire_unpack(p->ctx, blob.data() + hl, n1 + n2, words.data()));
    PvwCiphertext ct{std::vector<uint64_t>((size_t)p->k * P), std::vector<uint64_t>((size_t)p->n * P), p, rp};
    std::copy(words.begin(), words.begin() + n1 * P, ct.c1.begin() + (size_t)r[0] * P);
    std::copy(words.begin() + n1 * P, words.end(), ct.c2.begin() + (size_t)r[2] * P);
    return ct;
  }
};

// encrypt (encryption.rs:105-214)
inline PvwCiphertext encrypt(const std::vector<uint64_t>& scalars, const GlobalPublicKey& gpk, const Seed& seed,
                             uint32_t repr = PVW_REPR_NTT) {
  const auto& p = gpk.params;
  PvwCiphertext ct{std::vector<uint64_t>((size_t)p->k * p->poly_words()), std::vector<uint64_t>((size_t)p->n * p->poly_words()), p, repr};
  pvw_randomness_t rnd{};
  rnd.mode = PVW_RND_SEED;
  for (int i = 0; i < 32; ++i) rnd.seed[i] = seed[i];
  check(pvw_encrypt(p->ctx, scalars.data(), scalars.size(), &rnd, ct.c1.data(), ct.c2.data(), repr));
  ct.validate();                                                                                     // :204-211
  return ct;
}
// the same with the randomness drawn from a DeviceRandomness (call_seed(S, c); the state then holds c + 1)
inline PvwCiphertext encrypt(const std::vector<uint64_t>& scalars, const GlobalPublicKey& gpk, DeviceRandomness& rnd,
                             uint32_t repr = PVW_REPR_NTT) {
  const auto& p = gpk.params;
  PvwCiphertext ct{std::vector<uint64_t>((size_t)p->k * p->poly_words()), std::vector<uint64_t>((size_t)p->n * p->poly_words()), p, repr};
  check(pvw_encrypt_rs(p->ctx, scalars.data(), scalars.size(), rnd.raw(), ct.c1.data(), ct.c2.data(), repr));
  ct.validate();
  return ct;
}
inline Seed dealer_seed(Seed s, uint32_t dealer) {
  for (int i = 0; i < 4; ++i) s[28 + i] ^= (uint8_t)(dealer >> (8 * i));
  return s;
}
// encrypt_party_shares (encryption.rs:221-245)
inline PvwCiphertext encrypt_party_shares(const std::vector<uint64_t>& shares, uint32_t party_index,
                                          const GlobalPublicKey& gpk, const Seed& seed) {
  if (party_index >= gpk.params->n) throw PvwError(1, "Party index exceeds maximum");
  if (shares.size() != gpk.params->n) throw PvwError(1, "Party must provide n shares");
  return encrypt(shares, gpk, seed);
}
// encrypt_all_party_shares (encryption.rs:253-286): ONE batched call for all dealers (pvw_encrypt_multi: the
// dealers share passes over the public key; from 8 dealers up on the matrix cores), dealer d seeded with
// dealer_seed(seed, d) -- the same ciphertexts as n separate encrypt_party_shares calls
inline std::vector<PvwCiphertext> encrypt_all_party_shares(const std::vector<std::vector<uint64_t>>& all_shares,
                                                           const GlobalPublicKey& gpk, const Seed& seed,
                                                           uint32_t repr = PVW_REPR_NTT) {
  const auto& p = gpk.params;
  if (all_shares.size() != p->n) throw PvwError(1, "Must provide shares for all parties");
  const size_t D = all_shares.size(), n = p->n, P = p->poly_words();
  std::vector<uint64_t> scalars(D * n), c1(D * p->k * P), c2(D * n * P);
  std::vector<uint8_t> seeds(D * 32);
  for (size_t d = 0; d < D; ++d) {
    if (all_shares[d].size() != n) throw PvwError(1, "Party must provide n shares");
    std::copy(all_shares[d].begin(), all_shares[d].end(), scalars.begin() + d * n);
    const Seed sd = dealer_seed(seed, (uint32_t)d);
    std::copy(sd.begin(), sd.end(), seeds.begin() + d * 32);
  }
  check(pvw_encrypt_multi(p->ctx, scalars.data(), D, n, seeds.data(), c1.data(), c2.data(), repr));
  std::vector<PvwCiphertext> out;
  for (size_t d = 0; d < D; ++d) {
    PvwCiphertext ct{std::vector<uint64_t>(c1.begin() + d * p->k * P, c1.begin() + (d + 1) * p->k * P),
                     std::vector<uint64_t>(c2.begin() + d * n * P, c2.begin() + (d + 1) * n * P), p, repr};
    ct.validate();
    out.push_back(std::move(ct));
  }
  return out;
}
// ... with dealer d's randomness call_seed(S, c + d) of a DeviceRandomness (the state then holds c + n)
inline std::vector<PvwCiphertext> encrypt_all_party_shares(const std::vector<std::vector<uint64_t>>& all_shares,
                                                           const GlobalPublicKey& gpk, DeviceRandomness& rnd,
                                                           uint32_t repr = PVW_REPR_NTT) {
  const auto& p = gpk.params;
  if (all_shares.size() != p->n) throw PvwError(1, "Must provide shares for all parties");
  const size_t D = all_shares.size(), n = p->n, P = p->poly_words();
  std::vector<uint64_t> scalars(D * n), c1(D * p->k * P), c2(D * n * P);
  for (size_t d = 0; d < D; ++d) {
    if (all_shares[d].size() != n) throw PvwError(1, "Party must provide n shares");
    std::copy(all_shares[d].begin(), all_shares[d].end(), scalars.begin() + d * n);
  }
  check(pvw_encrypt_multi_rs(p->ctx, scalars.data(), D, n, rnd.raw(), c1.data(), c2.data(), repr));
  std::vector<PvwCiphertext> out;
  for (size_t d = 0; d < D; ++d) {
    PvwCiphertext ct{std::vector<uint64_t>(c1.begin() + d * p->k * P, c1.begin() + (d + 1) * p->k * P),
                     std::vector<uint64_t>(c2.begin() + d * n * P, c2.begin() + (d + 1) * n * P), p, repr};
    ct.validate();
    out.push_back(std::move(ct));
  }
  return out;
}
// encrypt_broadcast (encryption.rs:292-296)
inline PvwCiphertext encrypt_broadcast(uint64_t scalar, const GlobalPublicKey& gpk, const Seed& seed) {
  return encrypt(std::vector<uint64_t>(gpk.params->n, scalar), gpk, seed);
}
// decrypt_party_shares (decryption.rs:281-325): one batched device pass over all dealers
inline std::vector<uint64_t> decrypt_party_shares(const std::vector<PvwCiphertext>& cts, const SecretKey& sk, uint32_t party_index) {
  if (cts.empty()) throw PvwError(1, "No ciphertexts provided");
  const auto& p = cts[0].params;
  if (cts.size() != p->n) throw PvwError(1, "Expected n ciphertexts");
  if (party_index >= p->n) throw PvwError(1, "Party index exceeds maximum");
  const size_t P = p->poly_words();
  std::vector<uint64_t> c1s, c2col, out(cts.size());
  for (const auto& ct : cts) {
    ct.validate();
    c1s.insert(c1s.end(), ct.c1.begin(), ct.c1.end());
    c2col.insert(c2col.end(), ct.c2.begin() + (size_t)party_index * P, ct.c2.begin() + (size_t)(party_index + 1) * P);
  }
  check(pvw_decrypt_batch(p->ctx, sk.secret_coeffs.data(), c1s.data(), c2col.data(), cts.size(), cts[0].repr, out.data(), nullptr));
  return out;
}
// decrypt_party_shares with each share's report (pvw_decrypt_batch_checked): values as decrypt_party_shares,
// noise (max |residual|, saturating), lossy (the value is not the plaintext), valid = !lossy && noise <= bound
// plain (NULL or both fields 0: none): values = P mod plain->modulus and / or wide = plain->wide_words little-endian
// words of |P| per share (stored here; plain->wide is not used); valid then drops !lossy -- the values are exact -- and keeps the
// noise test; negative / truncated are the two further status bits
struct CheckedShares {
  std::vector<uint64_t> values, noise;
  std::vector<bool> lossy, valid;
  std::vector<bool> negative, truncated;
  std::vector<uint64_t> wide;
};
inline bool plain_on(const pvw_plain_t* plain) { return plain && (plain->modulus || plain->wide_words); }
inline void checked_report(CheckedShares& r, const std::vector<uint32_t>& status, uint64_t bound, bool plain) {
  const size_t n = status.size();
  r.negative.assign(n, false);
  r.truncated.assign(n, false);
  for (size_t d = 0; d < n; ++d) {
    r.lossy[d] = (status[d] & PVW_DEC_LOSSY) != 0;
    r.negative[d] = (status[d] & PVW_DEC_NEGATIVE) != 0;
    r.truncated[d] = (status[d] & PVW_DEC_WIDE_TRUNCATED) != 0;
    r.valid[d] = (plain || !r.lossy[d]) && r.noise[d] <= bound;
  }
}
inline CheckedShares decrypt_party_shares_checked(const std::vector<PvwCiphertext>& cts, const SecretKey& sk, uint32_t party_index,
                                                  uint64_t bound, const pvw_plain_t* plain = nullptr) {
  if (cts.empty()) throw PvwError(1, "No ciphertexts provided");
  const auto& p = cts[0].params;
  if (cts.size() != p->n) throw PvwError(1, "Expected n ciphertexts");
  if (party_index >= p->n) throw PvwError(1, "Party index exceeds maximum");
  const size_t P = p->poly_words(), D = cts.size();
  std::vector<uint64_t> c1s, c2col;
  std::vector<uint32_t> status(D);
  CheckedShares r{std::vector<uint64_t>(D), std::vector<uint64_t>(D), std::vector<bool>(D), std::vector<bool>(D)};
  for (const auto& ct : cts) {
    ct.validate();
    c1s.insert(c1s.end(), ct.c1.begin(), ct.c1.end());
    c2col.insert(c2col.end(), ct.c2.begin() + (size_t)party_index * P, ct.c2.begin() + (size_t)(party_index + 1) * P);
  }
  if (plain_on(plain)) {
    r.wide.assign(D * plain->wide_words, 0);
    check(pvw_decrypt_batch_plain(p->ctx, sk.secret_coeffs.data(), c1s.data(), c2col.data(), D, cts[0].repr, r.values.data(),
                                  r.noise.data(), status.data(), plain->modulus, plain->wide_words, r.wide.data()));
  } else {
    check(pvw_decrypt_batch_checked(p->ctx, sk.secret_coeffs.data(), c1s.data(), c2col.data(), D, cts[0].repr, r.values.data(),
                                    r.noise.data(), status.data()));
  }
  checked_report(r, status, bound, plain_on(plain));
  return r;
}
// the default bound of a checked decrypt: total_bound of verify_correctness_condition (parameters.rs:516-543)
inline uint64_t noise_bound(const pvw_ctx* ctx) {
  uint64_t b = 0;
  check(pvw_ctx_noise_bound(ctx, &b));
  return b;
}
// every party of [party_lo, party_lo + secret_keys.size()) decrypts its share of each ciphertext (any number of them, e.g.
// the valid subset of examples/pvw_valid_dec.rs:201-209) in one call (pvw_decrypt_all): result[p][d]
inline std::vector<std::vector<uint64_t>> decrypt_many(const std::vector<PvwCiphertext>& cts, const std::vector<const SecretKey*>& secret_keys,
                                                       uint32_t party_lo) {
  if (cts.empty()) throw PvwError(1, "No ciphertexts provided");
  const auto& p = cts[0].params;
  const size_t D = cts.size(), NP = secret_keys.size(), P = p->poly_words(), kl = (size_t)p->k * p->l;
  if (NP == 0) return {};
  std::vector<uint64_t> c1s, c2s, out(NP * D);
  c1s.reserve(D * p->k * P);
  c2s.reserve(D * p->n * P);
  for (const auto& ct : cts) {
    ct.validate();
    if (ct.repr != cts[0].repr) throw PvwError(1, "ciphertexts in different representations");
    c1s.insert(c1s.end(), ct.c1.begin(), ct.c1.end());
    c2s.insert(c2s.end(), ct.c2.begin(), ct.c2.end());
  }
  std::vector<int64_t> sk(NP * kl);
  for (size_t i = 0; i < NP; ++i) std::copy(secret_keys[i]->secret_coeffs.begin(), secret_keys[i]->secret_coeffs.end(), sk.begin() + i * kl);
  const int32_t rc = pvw_decrypt_all(p->ctx, party_lo, party_lo + (uint32_t)NP, sk.data(), c1s.data(), c2s.data(), D, cts[0].repr, out.data());
  std::fill(sk.begin(), sk.end(), 0);                                   // the copied keys do not outlive the call
  check(rc);
  std::vector<std::vector<uint64_t>> res(NP);
  for (size_t i = 0; i < NP; ++i) res[i].assign(out.begin() + i * D, out.begin() + (i + 1) * D);
  return res;
}
// the loop over decrypt_party_shares of examples/pvw.rs:138-149 as one call (an extension; no single reference function):
// results[recipient][dealer] (:157-170) for parties with consecutive indices, checks as decryption.rs:286-305
inline std::vector<std::vector<uint64_t>> decrypt_all_party_shares(const std::vector<PvwCiphertext>& cts, const std::vector<Party>& parties) {
  if (cts.empty()) throw PvwError(1, "No ciphertexts provided");
  const auto& p = cts[0].params;
  if (cts.size() != p->n) throw PvwError(1, "Expected " + std::to_string(p->n) + " ciphertexts, got " + std::to_string(cts.size()));
  if (parties.empty()) return {};
  std::vector<const SecretKey*> keys;
  for (size_t i = 0; i < parties.size(); ++i) {
    if (parties[i].index >= p->n)
      throw PvwError(1, "Party index " + std::to_string(parties[i].index) + " exceeds maximum " + std::to_string(p->n - 1));
    if (parties[i].index != parties[0].index + i) throw PvwError(1, "Party indices must be consecutive");
    keys.push_back(&parties[i].secret_key);
  }
  return decrypt_many(cts, keys, parties[0].index);
}
// decrypt_party_value (decryption.rs:249-278)
inline uint64_t decrypt_party_value(const PvwCiphertext& ct, const SecretKey& sk, uint32_t party_index) {
  const auto& p = ct.params;
  const size_t P = p->poly_words();
  uint64_t out = 0;
  check(pvw_decrypt_batch(p->ctx, sk.secret_coeffs.data(), ct.c1.data(), ct.c2.data() + (size_t)party_index * P, 1, ct.repr, &out, nullptr));
  return out;
}

// ---- sums of dealers' ciphertexts: the scheme is additively homomorphic, so party i's result of
// examples/pvw_valid_dec.rs:201-209 (the sum of its shares from the valid dealers) comes from ONE decrypt of the summed ciphertext
struct SumInputs {
  std::vector<uint64_t> c1s, c2s;
  std::vector<uint8_t> valid;      // empty = every dealer
  const uint8_t* valid_ptr() const { return valid.empty() ? nullptr : valid.data(); }
};
inline SumInputs sum_inputs(const std::vector<PvwCiphertext>& cts, const std::vector<bool>& valid) {
  if (cts.empty()) throw PvwError(1, "No ciphertexts provided");
  if (!valid.empty() && valid.size() != cts.size()) throw PvwError(PVW_ERR_DIMENSION_MISMATCH, "valid: one flag per ciphertext expected");
  SumInputs in;
  for (const auto& ct : cts) {
    if (ct.repr != cts[0].repr || ct.c1.size() != cts[0].c1.size() || ct.c2.size() != cts[0].c2.size())
      throw PvwError(PVW_ERR_DIMENSION_MISMATCH, "ciphertexts of different shapes or representations");
    ct.validate();
    in.c1s.insert(in.c1s.end(), ct.c1.begin(), ct.c1.end());
    in.c2s.insert(in.c2s.end(), ct.c2.begin(), ct.c2.end());
  }
  for (bool v : valid) in.valid.push_back(v ? 1 : 0);
  return in;
}
// ---- Shamir shares ----
// The bodies of shamir_shares / deal_party_shares and their packed forms (8.14).  pack == nullptr: the unpacked call, one secret
// per dealer; else secrets [D][*pack].  A deal takes seeds or, with seeds == nullptr, rnd.
inline size_t shamir_dealers(const std::vector<uint64_t>& secrets, const uint32_t* pack) {
  if (!pack) return secrets.size();
  if (*pack == 0 || secrets.size() % *pack) throw PvwError(15, "pack secrets per dealer");
  return secrets.size() / *pack;
}
inline std::vector<uint8_t> seed_bytes(const std::vector<Seed>& seeds) {
  std::vector<uint8_t> sd(seeds.size() * 32);
  for (size_t d = 0; d < seeds.size(); ++d) std::copy(seeds[d].begin(), seeds[d].end(), sd.begin() + d * 32);
  return sd;
}
inline std::vector<uint64_t> shamir_shares_call(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& secrets,
                                                const uint32_t* pack, uint32_t degree, uint64_t plain_modulus,
                                                const std::vector<Seed>& seeds, const std::vector<uint64_t>& coeffs, bool host) {
  const size_t D = shamir_dealers(secrets, pack);
  if (!seeds.empty() && seeds.size() != D) throw PvwError(15, "one seed per dealer");
  if (!coeffs.empty() && coeffs.size() != D * degree) throw PvwError(15, "degree coefficients per dealer");
  const std::vector<uint8_t> sd = seed_bytes(seeds);
  std::vector<uint64_t> out(D * p->n);
  const uint8_t* sdp = sd.empty() ? nullptr : sd.data();
  const uint64_t* cop = coeffs.empty() ? nullptr : coeffs.data();
  if (pack)
    check(host ? pvw_shamir_shares_packed_host(p->ctx, secrets.data(), D, *pack, degree, plain_modulus, sdp, cop, out.data())
               : pvw_shamir_shares_packed(p->ctx, secrets.data(), D, *pack, degree, plain_modulus, sdp, cop, out.data()));
  else
    check(host ? pvw_shamir_shares_host(p->ctx, secrets.data(), D, degree, plain_modulus, sdp, cop, out.data())
               : pvw_shamir_shares(p->ctx, secrets.data(), D, degree, plain_modulus, sdp, cop, out.data()));
  return out;
}
// shares[d][i] = f_d(i + 1) mod plain_modulus for dealer d's polynomial of `degree` with constant term secrets[d]; its other
// coefficients are drawn from seeds[d] (stream (PVW_DOM_SHAMIR << 32) | j) or given as coeffs [D][degree].  Row-major (D, n).
// On the device (pvw_shamir_shares); host = true: the plain C++ restatement (pvw_shamir_shares_host, no GPU).
inline std::vector<uint64_t> shamir_shares(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& secrets, uint32_t degree,
                                           uint64_t plain_modulus, const std::vector<Seed>& seeds,
                                           const std::vector<uint64_t>& coeffs = {}, bool host = false) {
  return shamir_shares_call(p, secrets, nullptr, degree, plain_modulus, seeds, coeffs, host);
}
inline std::vector<PvwCiphertext> deal_ciphertexts(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& c1,
                                                   const std::vector<uint64_t>& c2, size_t D, uint32_t repr) {
  const size_t n = p->n, P = p->poly_words();
  std::vector<PvwCiphertext> out;
  for (size_t d = 0; d < D; ++d)
    out.push_back(PvwCiphertext{std::vector<uint64_t>(c1.begin() + d * p->k * P, c1.begin() + (d + 1) * p->k * P),
                                std::vector<uint64_t>(c2.begin() + d * n * P, c2.begin() + (d + 1) * n * P), p, repr});
  return out;
}
inline std::vector<PvwCiphertext> deal_call(const std::vector<uint64_t>& secrets, const uint32_t* pack, uint32_t degree,
                                            uint64_t plain_modulus, const GlobalPublicKey& gpk, const std::vector<Seed>* seeds,
                                            DeviceRandomness* rnd, uint32_t out_repr) {
  const size_t D = shamir_dealers(secrets, pack);
  const auto& p = gpk.params;
  const size_t P = p->poly_words();
  if (seeds && seeds->size() != D) throw PvwError(15, "one seed per dealer");
  const std::vector<uint8_t> sd = seeds ? seed_bytes(*seeds) : std::vector<uint8_t>();
  std::vector<uint64_t> c1(D * p->k * P), c2(D * p->n * P);
  const uint64_t* se = secrets.data();
  if (seeds)
    check(pack ? pvw_deal_shares_packed(p->ctx, se, D, *pack, degree, plain_modulus, sd.data(), c1.data(), c2.data(), out_repr)
               : pvw_deal_shares(p->ctx, se, D, degree, plain_modulus, sd.data(), c1.data(), c2.data(), out_repr));
  else
    check(pack ? pvw_deal_shares_packed_rs(p->ctx, se, D, *pack, degree, plain_modulus, rnd->raw(), c1.data(), c2.data(), out_repr)
               : pvw_deal_shares_rs(p->ctx, se, D, degree, plain_modulus, rnd->raw(), c1.data(), c2.data(), out_repr));
  return deal_ciphertexts(p, c1, c2, D, out_repr);
}
// dealer d shares secrets[d] among the n parties and encrypts the shares in ONE device call (pvw_deal_shares): what
// encrypt of shamir_shares(...) under the same seeds returns, without the shares or coefficients existing on the host
inline std::vector<PvwCiphertext> deal_party_shares(const std::vector<uint64_t>& secrets, uint32_t degree, uint64_t plain_modulus,
                                                    const GlobalPublicKey& gpk, const std::vector<Seed>& seeds,
                                                    uint32_t out_repr = PVW_REPR_NTT) {
  return deal_call(secrets, nullptr, degree, plain_modulus, gpk, &seeds, nullptr, out_repr);
}
// ... with dealer d's randomness (polynomial and encryption) from call_seed(S, c + d) of a DeviceRandomness
inline std::vector<PvwCiphertext> deal_party_shares(const std::vector<uint64_t>& secrets, uint32_t degree, uint64_t plain_modulus,
                                                    const GlobalPublicKey& gpk, DeviceRandomness& rnd, uint32_t out_repr = PVW_REPR_NTT) {
  return deal_call(secrets, nullptr, degree, plain_modulus, gpk, nullptr, &rnd, out_repr);
}
// the secrets from the shares of the parties `indices` (at least degree + 1): shares [num_secrets][indices.size()], row-major
inline std::vector<uint64_t> shamir_reconstruct(const std::vector<uint64_t>& indices, const std::vector<uint64_t>& shares,
                                                uint64_t plain_modulus) {
  if (indices.empty() || shares.size() % indices.size()) throw PvwError(15, "shares must hold one value per index and secret");
  std::vector<uint64_t> out(shares.size() / indices.size());
  check(pvw_shamir_reconstruct(plain_modulus, indices.data(), shares.data(), indices.size(), out.size(), out.data()));
  return out;
}
// ---- Shamir shares over a prime below 2^256.  A wide element is four little-endian words; vectors of them are
// flat, four words per element.
using Wide = std::array<uint64_t, PVW_WIDE_WORDS>;
inline uint32_t shamir_wide_limbs(const Wide& plain_modulus, uint32_t limb_bits = 52) {
  uint32_t nl = 0;
  check(pvw_shamir_wide_limbs(plain_modulus.data(), limb_bits, &nl));
  return nl;
}
// shares [D][n][4] of secrets [D][4]; coefficients drawn from seeds[d] or given as coeffs [D][degree][4].  On the device
// (pvw_shamir_shares_wide); host = true: the restatement on the host cores (pvw_shamir_shares_wide_host, no GPU).
inline std::vector<uint64_t> shamir_shares_wide(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& secrets, uint32_t degree,
                                                const Wide& plain_modulus, const std::vector<Seed>& seeds,
                                                const std::vector<uint64_t>& coeffs = {}, bool host = false) {
  if (secrets.size() % PVW_WIDE_WORDS) throw PvwError(15, "four words per secret");
  const size_t D = secrets.size() / PVW_WIDE_WORDS;
  if (!seeds.empty() && seeds.size() != D) throw PvwError(15, "one seed per dealer");
  if (!coeffs.empty() && coeffs.size() != D * degree * PVW_WIDE_WORDS) throw PvwError(15, "degree coefficients per dealer");
  const std::vector<uint8_t> sd = seed_bytes(seeds);
  std::vector<uint64_t> out(D * p->n * PVW_WIDE_WORDS);
  const uint8_t* sdp = sd.empty() ? nullptr : sd.data();
  const uint64_t* cop = coeffs.empty() ? nullptr : coeffs.data();
  check(host ? pvw_shamir_shares_wide_host(p->ctx, secrets.data(), D, degree, plain_modulus.data(), sdp, cop, out.data())
             : pvw_shamir_shares_wide(p->ctx, secrets.data(), D, degree, plain_modulus.data(), sdp, cop, out.data()));
  return out;
}
inline std::vector<PvwCiphertext> deal_wide_call(const std::vector<uint64_t>& secrets, uint32_t degree, const Wide& plain_modulus,
                                                 const GlobalPublicKey& gpk, const std::vector<Seed>* seeds, DeviceRandomness* rnd,
                                                 uint32_t limb_bits, uint32_t out_repr) {
  if (secrets.size() % PVW_WIDE_WORDS) throw PvwError(15, "four words per secret");
  const size_t D = secrets.size() / PVW_WIDE_WORDS, V = D * shamir_wide_limbs(plain_modulus, limb_bits);
  const auto& p = gpk.params;
  const size_t P = p->poly_words();
  if (seeds && seeds->size() != V) throw PvwError(15, "one seed per limb ciphertext");
  const std::vector<uint8_t> sd = seeds ? seed_bytes(*seeds) : std::vector<uint8_t>();
  std::vector<uint64_t> c1(V * p->k * P), c2(V * p->n * P);
  if (seeds)
    check(pvw_deal_shares_wide(p->ctx, secrets.data(), D, degree, plain_modulus.data(), limb_bits, sd.data(), c1.data(), c2.data(), out_repr));
  else
    check(pvw_deal_shares_wide_rs(p->ctx, secrets.data(), D, degree, plain_modulus.data(), limb_bits, rnd->raw(), c1.data(), c2.data(), out_repr));
  return deal_ciphertexts(p, c1, c2, V, out_repr);
}
// dealer d shares secrets[d] and encrypts the shares limb by limb in ONE device call (pvw_deal_shares_wide): D * NL ciphertexts,
// ciphertext d * NL + w carrying limb w of dealer d's shares; seeds: one per ciphertext, dealer d draws under seeds[d * NL]
inline std::vector<PvwCiphertext> deal_party_shares_wide(const std::vector<uint64_t>& secrets, uint32_t degree, const Wide& plain_modulus,
                                                         const GlobalPublicKey& gpk, const std::vector<Seed>& seeds, uint32_t limb_bits = 52,
                                                         uint32_t out_repr = PVW_REPR_NTT) {
  return deal_wide_call(secrets, degree, plain_modulus, gpk, &seeds, nullptr, limb_bits, out_repr);
}
// ... with vector v's randomness from call_seed(S, c + v) of a DeviceRandomness, which then holds c + D * NL
inline std::vector<PvwCiphertext> deal_party_shares_wide(const std::vector<uint64_t>& secrets, uint32_t degree, const Wide& plain_modulus,
                                                         const GlobalPublicKey& gpk, DeviceRandomness& rnd, uint32_t limb_bits = 52,
                                                         uint32_t out_repr = PVW_REPR_NTT) {
  return deal_wide_call(secrets, degree, plain_modulus, gpk, nullptr, &rnd, limb_bits, out_repr);
}
// values [count][4] -> limbs [num_limbs][count], and back mod p (each input word any uint64_t: a limb or a sum of limbs)
inline std::vector<uint64_t> shamir_wide_to_limbs(const std::vector<uint64_t>& values, uint32_t limb_bits, uint32_t num_limbs) {
  const size_t count = values.size() / PVW_WIDE_WORDS;
  std::vector<uint64_t> out(count * num_limbs);
  check(pvw_shamir_wide_to_limbs_host(values.data(), count, limb_bits, num_limbs, out.data()));
  return out;
}
inline std::vector<uint64_t> shamir_wide_from_limbs(const Wide& plain_modulus, const std::vector<uint64_t>& limbs, uint32_t limb_bits,
                                                    uint32_t num_limbs) {
  if (!num_limbs || limbs.size() % num_limbs) throw PvwError(15, "limbs must hold num_limbs rows");
  const size_t count = limbs.size() / num_limbs;
  std::vector<uint64_t> out(count * PVW_WIDE_WORDS);
  check(pvw_shamir_wide_from_limbs_host(plain_modulus.data(), limbs.data(), count, limb_bits, num_limbs, out.data()));
  return out;
}
// the secrets [num_secrets][4] from shares [num_secrets][indices.size()][4] of the parties `indices` (at least degree + 1)
inline std::vector<uint64_t> shamir_reconstruct_wide(const std::vector<uint64_t>& indices, const std::vector<uint64_t>& shares,
                                                     const Wide& plain_modulus) {
  if (indices.empty() || shares.size() % (indices.size() * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and secret");
  const size_t S = shares.size() / (indices.size() * PVW_WIDE_WORDS);
  std::vector<uint64_t> out(S * PVW_WIDE_WORDS);
  check(pvw_shamir_reconstruct_wide(plain_modulus.data(), indices.data(), shares.data(), indices.size(), S, out.data()));
  return out;
}
// ---- the receiving end over a prime below 2^256 ----
// shamir_wide_from_limbs where the limbs lie (pvw_shamir_wide_from_limbs_device): device pointers, count elements [count][4] at
// d_out, asynchronous on `stream` (NULL: the context's).  Strides (count, 1) read limb planes, (1, num_limbs) the
// [party][dealer * NL + w] result of a decrypt-all in place.
inline void shamir_wide_from_limbs_device(const std::shared_ptr<PvwParameters>& p, const Wide& plain_modulus, const uint64_t* d_limbs,
                                          size_t count, size_t limb_stride, size_t elem_stride, uint32_t limb_bits, uint32_t num_limbs,
                                          uint64_t* d_out, void* stream = nullptr) {
  check(pvw_shamir_wide_from_limbs_device(p->ctx, plain_modulus.data(), d_limbs, count, limb_stride, elem_stride, limb_bits, num_limbs,
                                          d_out, stream));
}
struct CheckedWideSecrets {
  std::vector<uint64_t> secrets;    // [num_secrets][4]: the value at 0 of the polynomial through each secret's basis shares
  std::vector<uint32_t> bad;        // [num_secrets]: columns beyond the basis whose share is off that polynomial
  std::vector<uint32_t> col_bad;    // [indices.size()]: secrets that deviate in each column (0 for the basis columns)
};
// shamir_reconstruct_checked over an odd prime below 2^256.  The first degree + 1 of `indices` are the basis.  shares
// [num_secrets][indices.size()][4] row-major, or party_major [indices.size()][num_secrets][4]; any words, read mod p.  On the
// device (pvw_shamir_reconstruct_wide_checked); host = true: the plain C++ restatement (no GPU; p may be null).
inline CheckedWideSecrets shamir_reconstruct_wide_checked(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                          const std::vector<uint64_t>& shares, uint32_t degree, const Wide& plain_modulus,
                                                          bool party_major = false, bool host = false) {
  const size_t count = indices.size();
  if (count == 0 || shares.empty() || shares.size() % (count * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and secret");
  const size_t S = shares.size() / (count * PVW_WIDE_WORDS), ss = party_major ? 1 : count, ps = party_major ? S : 1;
  CheckedWideSecrets r{std::vector<uint64_t>(S * PVW_WIDE_WORDS), std::vector<uint32_t>(S), std::vector<uint32_t>(count)};
  check(host ? pvw_shamir_reconstruct_wide_checked_host(plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps,
                                                        r.secrets.data(), r.bad.data(), r.col_bad.data())
             : pvw_shamir_reconstruct_wide_checked(p->ctx, plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps,
                                                   r.secrets.data(), r.bad.data(), r.col_bad.data()));
  return r;
}
// ---- corrected reconstruction over an odd prime below 2^256 ----
struct CorrectedWideSecrets {
  std::vector<uint64_t> secrets;    // [num_secrets][4]: the value at 0 of the one polynomial within E columns of the row; 0: undecodable
  std::vector<uint32_t> nerr;       // [num_secrets]: columns off that polynomial, or PVW_SHAMIR_UNDECODABLE
  std::vector<uint32_t> col_err;    // [indices.size()]: decodable secrets that are off in each column
  std::vector<uint64_t> err_mask;   // [num_secrets][words]: bit c % 64 of word c / 64 names the columns of nerr
  size_t words;                     // ceil(indices.size() / 64)
  bool wrong(size_t s, size_t c) const { return (err_mask[s * words + c / 64] >> (c % 64)) & 1; }
};
// Up to E = (indices.size() - degree - 1) / 2 wrong shares per secret, in whichever columns.  shares as
// shamir_reconstruct_wide_checked.  On the device (pvw_shamir_reconstruct_wide_corrected); host = true: the plain C++ restatement
// (Berlekamp-Welch, no GPU; p may be null).
inline CorrectedWideSecrets shamir_reconstruct_wide_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                              const std::vector<uint64_t>& shares, uint32_t degree, const Wide& plain_modulus,
                                                              bool party_major = false, bool host = false) {
  const size_t count = indices.size();
  if (count == 0 || shares.empty() || shares.size() % (count * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and secret");
  const size_t S = shares.size() / (count * PVW_WIDE_WORDS), ss = party_major ? 1 : count, ps = party_major ? S : 1;
  const size_t words = (count + 63) / 64;
  CorrectedWideSecrets r{std::vector<uint64_t>(S * PVW_WIDE_WORDS), std::vector<uint32_t>(S), std::vector<uint32_t>(count),
                         std::vector<uint64_t>(S * words), words};
  check(host ? pvw_shamir_reconstruct_wide_corrected_host(plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps,
                                                          r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data())
             : pvw_shamir_reconstruct_wide_corrected(p->ctx, plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps,
                                                     r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data()));
  return r;
}
// ---- reconstruction with erasures over an odd prime below 2^256 ----
// The call above with `erased` [num_secrets][words] in the layout of CorrectedWideSecrets::err_mask (bit c % 64 of word c / 64 of
// row s: share (s, c) is known to be bad).  An erased share costs one redundant column instead of two: a row decodes while
// 2 errors + erasures <= indices.size() - degree - 1; the words at an erased position influence nothing and an erased column is
// never reported as an error.  An empty `erased` is the call above.
inline CorrectedWideSecrets shamir_reconstruct_wide_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                              const std::vector<uint64_t>& shares, uint32_t degree, const Wide& plain_modulus,
                                                              const std::vector<uint64_t>& erased, bool party_major, bool host = false) {
  const size_t count = indices.size();
  if (count == 0 || shares.empty() || shares.size() % (count * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and secret");
  const size_t S = shares.size() / (count * PVW_WIDE_WORDS), ss = party_major ? 1 : count, ps = party_major ? S : 1;
  const size_t words = (count + 63) / 64;
  if (!erased.empty() && erased.size() != S * words) throw PvwError(15, "erased must hold ceil(count / 64) words per secret");
  const uint64_t* er = erased.empty() ? nullptr : erased.data();
  CorrectedWideSecrets r{std::vector<uint64_t>(S * PVW_WIDE_WORDS), std::vector<uint32_t>(S), std::vector<uint32_t>(count),
                         std::vector<uint64_t>(S * words), words};
  check(host ? pvw_shamir_reconstruct_wide_erasures_host(plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                                         r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data())
             : pvw_shamir_reconstruct_wide_erasures(p->ctx, plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps,
                                                    er, r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data()));
  return r;
}
// ---- share repair over an odd prime below 2^256 ----
struct EvaluatedWideShares {
  std::vector<uint64_t> values;     // [num_secrets][targets.size()][4]: F_s(targets[j] + 1); the row of an undecodable secret is 0
  CorrectedWideSecrets report;      // what shamir_reconstruct_wide_corrected returns on the same input
};
// The decode of shamir_reconstruct_wide_corrected and the corrected polynomials at the points of the parties `targets` (global
// indices whose point targets[j] + 1 is below p: columns of the call -- the share that party should hold -- or any other;
// duplicates allowed).  `erased` as in the overload above; empty: no mask.  On the device (pvw_shamir_evaluate_wide_corrected /
// _erasures); host = true: the plain C++ restatement (no GPU; p may be null).
inline EvaluatedWideShares shamir_evaluate_wide_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                          const std::vector<uint64_t>& shares, uint32_t degree, const Wide& plain_modulus,
                                                          const std::vector<uint64_t>& targets, const std::vector<uint64_t>& erased = {},
                                                          bool party_major = false, bool host = false) {
  const size_t count = indices.size(), T = targets.size();
  if (count == 0 || shares.empty() || shares.size() % (count * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and secret");
  const size_t S = shares.size() / (count * PVW_WIDE_WORDS), ss = party_major ? 1 : count, ps = party_major ? S : 1;
  const size_t words = (count + 63) / 64;
  if (!erased.empty() && erased.size() != S * words) throw PvwError(15, "erased must hold ceil(count / 64) words per secret");
  const uint64_t* er = erased.empty() ? nullptr : erased.data();
  EvaluatedWideShares r{std::vector<uint64_t>(S * T * PVW_WIDE_WORDS),
                        CorrectedWideSecrets{std::vector<uint64_t>(S * PVW_WIDE_WORDS), std::vector<uint32_t>(S), std::vector<uint32_t>(count),
                                             std::vector<uint64_t>(S * words), words}};
  CorrectedWideSecrets& c = r.report;
  check(host ? pvw_shamir_evaluate_wide_erasures_host(plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                                      targets.data(), T, r.values.data(), c.secrets.data(), c.nerr.data(), c.col_err.data(),
                                                      c.err_mask.data())
             : pvw_shamir_evaluate_wide_erasures(p->ctx, plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                                 targets.data(), T, r.values.data(), c.secrets.data(), c.nerr.data(), c.col_err.data(),
                                                 c.err_mask.data()));
  return r;
}
// ---- packed dealing over an odd prime below 2^256 ----
// shares [D][n][4] of secrets [D][pack][4], dealer-major: `pack` secrets at the points 0, -1, .., -(pack-1) of one polynomial with
// `degree` random coefficients, drawn from seeds[d] or given as coeffs [D][degree][4].  On the device
// (pvw_shamir_shares_packed_wide); host = true: the restatement on the host cores (no GPU).  pack = 1 is shamir_shares_wide.
inline std::vector<uint64_t> shamir_shares_packed_wide(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& secrets,
                                                       uint32_t pack, uint32_t degree, const Wide& plain_modulus, const std::vector<Seed>& seeds,
                                                       const std::vector<uint64_t>& coeffs = {}, bool host = false) {
  if (!pack || secrets.size() % ((size_t)pack * PVW_WIDE_WORDS)) throw PvwError(15, "pack elements of four words per dealer");
  const size_t D = secrets.size() / ((size_t)pack * PVW_WIDE_WORDS);
  if (!seeds.empty() && seeds.size() != D) throw PvwError(15, "one seed per dealer");
  if (!coeffs.empty() && coeffs.size() != D * degree * PVW_WIDE_WORDS) throw PvwError(15, "degree coefficients per dealer");
  const std::vector<uint8_t> sd = seed_bytes(seeds);
  std::vector<uint64_t> out(D * p->n * PVW_WIDE_WORDS);
  const uint8_t* sdp = sd.empty() ? nullptr : sd.data();
  const uint64_t* cop = coeffs.empty() ? nullptr : coeffs.data();
  check(host ? pvw_shamir_shares_packed_wide_host(p->ctx, secrets.data(), D, pack, degree, plain_modulus.data(), sdp, cop, out.data())
             : pvw_shamir_shares_packed_wide(p->ctx, secrets.data(), D, pack, degree, plain_modulus.data(), sdp, cop, out.data()));
  return out;
}
inline std::vector<PvwCiphertext> deal_packed_wide_call(const std::vector<uint64_t>& secrets, uint32_t pack, uint32_t degree,
                                                        const Wide& plain_modulus, const GlobalPublicKey& gpk, const std::vector<Seed>* seeds,
                                                        DeviceRandomness* rnd, uint32_t limb_bits, uint32_t out_repr) {
  if (!pack || secrets.size() % ((size_t)pack * PVW_WIDE_WORDS)) throw PvwError(15, "pack elements of four words per dealer");
  const size_t D = secrets.size() / ((size_t)pack * PVW_WIDE_WORDS), V = D * shamir_wide_limbs(plain_modulus, limb_bits);
  const auto& p = gpk.params;
  const size_t P = p->poly_words();
  if (seeds && seeds->size() != V) throw PvwError(15, "one seed per limb ciphertext");
  const std::vector<uint8_t> sd = seeds ? seed_bytes(*seeds) : std::vector<uint8_t>();
  std::vector<uint64_t> c1(V * p->k * P), c2(V * p->n * P);
  if (seeds)
    check(pvw_deal_shares_packed_wide(p->ctx, secrets.data(), D, pack, degree, plain_modulus.data(), limb_bits, sd.data(), c1.data(), c2.data(),
                                      out_repr));
  else
    check(pvw_deal_shares_packed_wide_rs(p->ctx, secrets.data(), D, pack, degree, plain_modulus.data(), limb_bits, rnd->raw(), c1.data(),
                                         c2.data(), out_repr));
  return deal_ciphertexts(p, c1, c2, V, out_repr);
}
// deal_party_shares_wide with `pack` secrets per dealer in one polynomial (pvw_deal_shares_packed_wide): D * NL ciphertexts carry
// D * pack wide secrets; seeds and limbs as deal_party_shares_wide
inline std::vector<PvwCiphertext> deal_party_shares_packed_wide(const std::vector<uint64_t>& secrets, uint32_t pack, uint32_t degree,
                                                                const Wide& plain_modulus, const GlobalPublicKey& gpk,
                                                                const std::vector<Seed>& seeds, uint32_t limb_bits = 52,
                                                                uint32_t out_repr = PVW_REPR_NTT) {
  return deal_packed_wide_call(secrets, pack, degree, plain_modulus, gpk, &seeds, nullptr, limb_bits, out_repr);
}
// ... with vector v's randomness from call_seed(S, c + v) of a DeviceRandomness, which then holds c + D * NL
inline std::vector<PvwCiphertext> deal_party_shares_packed_wide(const std::vector<uint64_t>& secrets, uint32_t pack, uint32_t degree,
                                                                const Wide& plain_modulus, const GlobalPublicKey& gpk, DeviceRandomness& rnd,
                                                                uint32_t limb_bits = 52, uint32_t out_repr = PVW_REPR_NTT) {
  return deal_packed_wide_call(secrets, pack, degree, plain_modulus, gpk, nullptr, &rnd, limb_bits, out_repr);
}
// out [num_rows][pack][4]: every row's values at 0, -1, .., -(pack-1) from shares [num_rows][indices.size()][4] of the parties
// `indices` (at least degree + pack of them); host only (pvw_shamir_reconstruct_packed_wide)
inline std::vector<uint64_t> shamir_reconstruct_packed_wide(const std::vector<uint64_t>& indices, const std::vector<uint64_t>& shares,
                                                            const Wide& plain_modulus, uint32_t pack) {
  if (indices.empty() || shares.size() % (indices.size() * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and row");
  const size_t R = shares.size() / (indices.size() * PVW_WIDE_WORDS);
  std::vector<uint64_t> out(R * (pack ? pack : 1) * PVW_WIDE_WORDS);
  check(pvw_shamir_reconstruct_packed_wide(plain_modulus.data(), pack, indices.data(), shares.data(), indices.size(), R, out.data()));
  return out;
}
struct CorrectedPackedWideSecrets {
  std::vector<uint64_t> secrets;    // [num_rows][pack][4]; the row of an undecodable sharing is 0
  CorrectedWideSecrets report;      // the decode's report, unchanged
};
// The secrets of a packed wide sharing although up to (indices.size() - degree - pack) / 2 shares of each row are wrong.  The wide
// evaluate calls take targets as party indices, so the points -j cannot be named for a wide p: ONE shamir_evaluate_wide_corrected
// call at polynomial degree degree + pack - 1 evaluates the corrected polynomials at the first degree + pack of `indices`, and
// shamir_reconstruct_packed_wide reads the secrets off those corrected shares.  pack = 1: shamir_reconstruct_wide_corrected.
inline CorrectedPackedWideSecrets shamir_reconstruct_packed_wide_corrected(const std::shared_ptr<PvwParameters>& p, const Wide& plain_modulus,
                                                                           uint32_t pack, uint32_t degree, const std::vector<uint64_t>& indices,
                                                                           const std::vector<uint64_t>& shares,
                                                                           const std::vector<uint64_t>& erased = {}, bool party_major = false,
                                                                           bool host = false) {
  if (pack == 0) throw PvwError(1, "pack must be at least 1");
  if (pack == 1) {
    CorrectedWideSecrets r = shamir_reconstruct_wide_corrected(p, indices, shares, degree, plain_modulus, erased, party_major, host);
    std::vector<uint64_t> secrets = r.secrets;
    return CorrectedPackedWideSecrets{std::move(secrets), std::move(r)};
  }
  const size_t need = (size_t)degree + pack;
  if (indices.size() < need) throw PvwError(1, "degree + pack shares are needed");
  const std::vector<uint64_t> basis(indices.begin(), indices.begin() + need);
  EvaluatedWideShares ev = shamir_evaluate_wide_corrected(p, indices, shares, degree + pack - 1, plain_modulus, basis, erased, party_major, host);
  std::vector<uint64_t> secrets = shamir_reconstruct_packed_wide(basis, ev.values, plain_modulus, pack);
  for (size_t r = 0; r < ev.report.nerr.size(); ++r)
    if (ev.report.nerr[r] == PVW_SHAMIR_UNDECODABLE)
      std::fill(secrets.begin() + r * pack * PVW_WIDE_WORDS, secrets.begin() + (r + 1) * pack * PVW_WIDE_WORDS, (uint64_t)0);
  return CorrectedPackedWideSecrets{std::move(secrets), std::move(ev.report)};
}
// ---- wide share repair at field points ----
// shamir_evaluate_wide_corrected with the point of column j of values given as the field element points[j] (points holds four
// little-endian words per point, each point below p): 0, points above 2^64 and points on columns are legal; at the point 0 the
// value is the secret.  (pvw_shamir_evaluate_wide_erasures_at / _at_host)
inline EvaluatedWideShares shamir_evaluate_wide_corrected_at(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                             const std::vector<uint64_t>& shares, uint32_t degree, const Wide& plain_modulus,
                                                             const std::vector<uint64_t>& points, const std::vector<uint64_t>& erased = {},
                                                             bool party_major = false, bool host = false) {
  const size_t count = indices.size();
  if (points.size() % PVW_WIDE_WORDS) throw PvwError(15, "points must hold four words per point");
  const size_t T = points.size() / PVW_WIDE_WORDS;
  if (count == 0 || shares.empty() || shares.size() % (count * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and secret");
  const size_t S = shares.size() / (count * PVW_WIDE_WORDS), ss = party_major ? 1 : count, ps = party_major ? S : 1;
  const size_t words = (count + 63) / 64;
  if (!erased.empty() && erased.size() != S * words) throw PvwError(15, "erased must hold ceil(count / 64) words per secret");
  const uint64_t* er = erased.empty() ? nullptr : erased.data();
  EvaluatedWideShares r{std::vector<uint64_t>(S * T * PVW_WIDE_WORDS),
                        CorrectedWideSecrets{std::vector<uint64_t>(S * PVW_WIDE_WORDS), std::vector<uint32_t>(S), std::vector<uint32_t>(count),
                                             std::vector<uint64_t>(S * words), words}};
  CorrectedWideSecrets& c = r.report;
  check(host ? pvw_shamir_evaluate_wide_erasures_at_host(plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                                         points.data(), T, r.values.data(), c.secrets.data(), c.nerr.data(),
                                                         c.col_err.data(), c.err_mask.data())
             : pvw_shamir_evaluate_wide_erasures_at(p->ctx, plain_modulus.data(), degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                                    points.data(), T, r.values.data(), c.secrets.data(), c.nerr.data(), c.col_err.data(),
                                                    c.err_mask.data()));
  return r;
}
// The secrets [num_rows][pack][4] of a packed wide sharing in ONE call, with shares wrong or erased: the rows are decoded at
// polynomial degree degree + pack - 1 and read at the points -m (pvw_shamir_packed_wide_secrets / _host).  The report's `secrets`
// stays empty: the secrets of a packed row are the first member.  Every index must be below p - pack.
inline CorrectedPackedWideSecrets shamir_packed_wide_secrets(const std::shared_ptr<PvwParameters>& p, const Wide& plain_modulus, uint32_t pack,
                                                             uint32_t degree, const std::vector<uint64_t>& indices,
                                                             const std::vector<uint64_t>& shares, const std::vector<uint64_t>& erased = {},
                                                             bool party_major = false, bool host = false) {
  const size_t count = indices.size();
  if (count == 0 || shares.empty() || shares.size() % (count * PVW_WIDE_WORDS)) throw PvwError(15, "shares must hold one element per index and row");
  const size_t S = shares.size() / (count * PVW_WIDE_WORDS), ss = party_major ? 1 : count, ps = party_major ? S : 1;
  const size_t words = (count + 63) / 64;
  if (!erased.empty() && erased.size() != S * words) throw PvwError(15, "erased must hold ceil(count / 64) words per row");
  const uint64_t* er = erased.empty() ? nullptr : erased.data();
  CorrectedPackedWideSecrets r{std::vector<uint64_t>(S * (pack ? pack : 1) * PVW_WIDE_WORDS),
                               CorrectedWideSecrets{{}, std::vector<uint32_t>(S), std::vector<uint32_t>(count),
                                                    std::vector<uint64_t>(S * words), words}};
  CorrectedWideSecrets& c = r.report;
  check(host ? pvw_shamir_packed_wide_secrets_host(plain_modulus.data(), pack, degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                                   r.secrets.data(), c.nerr.data(), c.col_err.data(), c.err_mask.data())
             : pvw_shamir_packed_wide_secrets(p->ctx, plain_modulus.data(), pack, degree, indices.data(), count, shares.data(), S, ss, ps, er,
                                              r.secrets.data(), c.nerr.data(), c.col_err.data(), c.err_mask.data()));
  return r;
}
// The mask of wide shares from a per-limb decrypt report on the host (pvw_shamir_wide_erasure_mask_host): status / noise
// [num_secrets][count * num_limbs], or with party_major [count][num_secrets * num_limbs] (the [party][dealer NL + w] report of the
// decrypt-all calls); either may be empty, not both.  Share (s, c) is erased iff one of its limbs has status & status_bits or
// noise > noise_bound.
inline std::vector<uint64_t> shamir_wide_erasure_mask(const std::vector<uint32_t>& status, const std::vector<uint64_t>& noise, size_t count,
                                                      uint32_t num_limbs, uint32_t status_bits, uint64_t noise_bound,
                                                      bool party_major = false) {
  const size_t cells = status.empty() ? noise.size() : status.size();
  if (count == 0 || num_limbs == 0 || cells == 0 || cells % (count * num_limbs) ||
      (!status.empty() && !noise.empty() && status.size() != noise.size()))
    throw PvwError(15, "status and noise must hold num_limbs values per share");
  const size_t S = cells / (count * num_limbs), NL = num_limbs;
  std::vector<uint64_t> mask(S * ((count + 63) / 64));
  check(pvw_shamir_wide_erasure_mask_host(status.empty() ? nullptr : const_cast<uint32_t*>(status.data()) /* only read */,
                                          noise.empty() ? nullptr : noise.data(), status_bits, noise_bound, count, S,
                                          party_major ? NL : count * NL, party_major ? S * NL : NL, num_limbs, 1, mask.data()));
  return mask;
}
// the share matrix of the checked, corrected and evaluate calls: its shape and the strides of its layout, in words
struct ShareMatrix {
  size_t count, S, words, ss, ps;   // columns, secrets, mask words per secret, secret stride, point stride
  ShareMatrix(const std::vector<uint64_t>& indices, const std::vector<uint64_t>& shares, bool party_major) : count(indices.size()) {
    if (count == 0 || shares.empty() || shares.size() % count) throw PvwError(15, "shares must hold one value per index and secret");
    S = shares.size() / count, words = (count + 63) / 64;
    ss = party_major ? 1 : count, ps = party_major ? S : 1;
  }
};
// ---- checked reconstruction ----
struct CheckedSecrets {
  std::vector<uint64_t> secrets;    // [num_secrets]: the value at 0 of the polynomial through each secret's basis shares
  std::vector<uint32_t> bad;        // [num_secrets]: columns beyond the basis whose share is off that polynomial
  std::vector<uint32_t> col_bad;    // [indices.size()]: secrets that deviate in each column (0 for the basis columns)
};
// The first degree + 1 of `indices` are the basis.  shares: party_major = false: [num_secrets][indices.size()] (the rows of
// shamir_shares); true: [indices.size()][num_secrets] (what decrypt_all_party_shares* returns, every dealer a secret).
// On the device (pvw_shamir_reconstruct_checked); host = true: the plain C++ restatement (no GPU, p may be null).
inline CheckedSecrets shamir_reconstruct_checked(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                 const std::vector<uint64_t>& shares, uint32_t degree, uint64_t plain_modulus,
                                                 bool host = false, bool party_major = false) {
  const ShareMatrix m(indices, shares, party_major);
  CheckedSecrets r{std::vector<uint64_t>(m.S), std::vector<uint32_t>(m.S), std::vector<uint32_t>(m.count)};
  check(host ? pvw_shamir_reconstruct_checked_host(plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps,
                                                   r.secrets.data(), r.bad.data(), r.col_bad.data())
             : pvw_shamir_reconstruct_checked(p->ctx, plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps,
                                              r.secrets.data(), r.bad.data(), r.col_bad.data()));
  return r;
}

// ---- corrected reconstruction ----
struct CorrectedSecrets {
  std::vector<uint64_t> secrets;    // [num_secrets]: the value at 0 of the one polynomial within E columns of the row; 0: undecodable
  std::vector<uint32_t> nerr;       // [num_secrets]: columns off that polynomial, or PVW_SHAMIR_UNDECODABLE
  std::vector<uint32_t> col_err;    // [indices.size()]: decodable secrets that are off in each column
  std::vector<uint64_t> err_mask;   // [num_secrets][words]: bit c % 64 of word c / 64 names the columns of nerr
  size_t words;                     // ceil(indices.size() / 64)
  bool wrong(size_t s, size_t c) const { return (err_mask[s * words + c / 64] >> (c % 64)) & 1; }
};
inline CorrectedSecrets corrected_report(const ShareMatrix& m) {   // all 0, of the matrix's shape
  return {std::vector<uint64_t>(m.S), std::vector<uint32_t>(m.S), std::vector<uint32_t>(m.count), std::vector<uint64_t>(m.S * m.words), m.words};
}
// Up to E = (indices.size() - degree - 1) / 2 wrong shares per secret, in whichever columns.  shares as shamir_reconstruct_checked.
// On the device (pvw_shamir_reconstruct_corrected); host = true: the plain C++ restatement (no GPU, p may be null).
inline CorrectedSecrets shamir_reconstruct_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                     const std::vector<uint64_t>& shares, uint32_t degree, uint64_t plain_modulus,
                                                     bool host = false, bool party_major = false) {
  const ShareMatrix m(indices, shares, party_major);
  CorrectedSecrets r = corrected_report(m);
  check(host ? pvw_shamir_reconstruct_corrected_host(plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps,
                                                     r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data())
             : pvw_shamir_reconstruct_corrected(p->ctx, plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps,
                                                r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data()));
  return r;
}

// ---- share repair ----
struct EvaluatedShares {
  std::vector<uint64_t> values;     // [num_secrets][targets.size()]: the corrected polynomial of each row at each target's point; a 0 row: undecodable
  CorrectedSecrets decode;          // what shamir_reconstruct_corrected reports for the same input
};
// The decode of shamir_reconstruct_corrected and its polynomials at the points of the parties `targets` (global indices: among
// `indices` or not, duplicates allowed).  On the device (pvw_shamir_evaluate_corrected); host = true: the plain C++ restatement.
inline EvaluatedShares shamir_evaluate_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                 const std::vector<uint64_t>& shares, uint32_t degree, uint64_t plain_modulus,
                                                 const std::vector<uint64_t>& targets, bool host = false, bool party_major = false) {
  const ShareMatrix m(indices, shares, party_major);
  const size_t T = targets.size();
  EvaluatedShares r{std::vector<uint64_t>(m.S * T), corrected_report(m)};
  CorrectedSecrets& d = r.decode;
  check(host ? pvw_shamir_evaluate_corrected_host(plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps, targets.data(),
                                                  T, r.values.data(), d.secrets.data(), d.nerr.data(), d.col_err.data(), d.err_mask.data())
             : pvw_shamir_evaluate_corrected(p->ctx, plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps,
                                             targets.data(), T, r.values.data(), d.secrets.data(), d.nerr.data(), d.col_err.data(),
                                             d.err_mask.data()));
  return r;
}

// ---- reconstruction with erasures ----
// The calls above with `erased` [num_secrets][words] in the layout of CorrectedSecrets::err_mask (bit c % 64 of word c / 64 of row
// s: share (s, c) is known to be bad).  An erased share costs one redundant column instead of two: a row decodes while
// 2 errors + erasures <= indices.size() - degree - 1; the word at an erased position influences nothing and an erased column is never
// reported as an error.  An empty `erased` is the call above.
inline const uint64_t* erased_rows(const ShareMatrix& m, const std::vector<uint64_t>& erased) {
  if (erased.empty()) return nullptr;
  if (erased.size() != m.S * m.words) throw PvwError(15, "erased must hold ceil(count / 64) words per secret");
  return erased.data();
}
inline CorrectedSecrets shamir_reconstruct_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                     const std::vector<uint64_t>& shares, uint32_t degree, uint64_t plain_modulus,
                                                     const std::vector<uint64_t>& erased, bool host, bool party_major = false) {
  const ShareMatrix m(indices, shares, party_major);
  const uint64_t* er = erased_rows(m, erased);
  CorrectedSecrets r = corrected_report(m);
  check(host ? pvw_shamir_reconstruct_erasures_host(plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps, er,
                                                    r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data())
             : pvw_shamir_reconstruct_erasures(p->ctx, plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps, er,
                                               r.secrets.data(), r.nerr.data(), r.col_err.data(), r.err_mask.data()));
  return r;
}
// At an erased or wrong column the value is the share that party should hold: the repair of a party that lost its state.
inline EvaluatedShares shamir_evaluate_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                 const std::vector<uint64_t>& shares, uint32_t degree, uint64_t plain_modulus,
                                                 const std::vector<uint64_t>& targets, const std::vector<uint64_t>& erased, bool host,
                                                 bool party_major = false) {
  const ShareMatrix m(indices, shares, party_major);
  const uint64_t* er = erased_rows(m, erased);
  const size_t T = targets.size();
  EvaluatedShares r{std::vector<uint64_t>(m.S * T), corrected_report(m)};
  CorrectedSecrets& d = r.decode;
  check(host ? pvw_shamir_evaluate_erasures_host(plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps, er,
                                                 targets.data(), T, r.values.data(), d.secrets.data(), d.nerr.data(), d.col_err.data(),
                                                 d.err_mask.data())
             : pvw_shamir_evaluate_erasures(p->ctx, plain_modulus, degree, indices.data(), m.count, shares.data(), m.S, m.ss, m.ps, er,
                                            targets.data(), T, r.values.data(), d.secrets.data(), d.nerr.data(), d.col_err.data(),
                                            d.err_mask.data()));
  return r;
}
// The mask of a decrypt report on the host (pvw_shamir_erasure_mask_host): status / noise [num_secrets][count], or with party_major
// [count][num_secrets]; either may be empty, not both.  Share (s, c) is erased iff status & status_bits or noise > noise_bound.
inline std::vector<uint64_t> shamir_erasure_mask(const std::vector<uint32_t>& status, const std::vector<uint64_t>& noise, size_t count,
                                                 uint32_t status_bits, uint64_t noise_bound, bool party_major = false) {
  const size_t cells = status.empty() ? noise.size() : status.size();
  if (count == 0 || cells == 0 || cells % count || (!status.empty() && !noise.empty() && status.size() != noise.size()))
    throw PvwError(15, "status and noise must hold one value per share");
  const size_t S = cells / count;
  std::vector<uint64_t> mask(S * ((count + 63) / 64));
  check(pvw_shamir_erasure_mask_host(status.empty() ? nullptr : const_cast<uint32_t*>(status.data()) /* only read */, noise.empty() ? nullptr : noise.data(), status_bits,
                                     noise_bound, count, S, party_major ? 1 : count, party_major ? S : 1, mask.data()));
  return mask;
}

// ---- packed sharing ----
// secrets [D][pack] row-major: dealer d's `pack` secrets sit at the points 0, -1, ..., -(pack-1) of one polynomial with `degree`
// random coefficients (drawn as shamir_shares draws them, or coeffs [D][degree]); shares (D, n) row-major.  pack = 1 is
// shamir_shares.  On the device (pvw_shamir_shares_packed); host = true: the plain C++ restatement (no GPU).
inline std::vector<uint64_t> shamir_shares_packed(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& secrets,
                                                  uint32_t pack, uint32_t degree, uint64_t plain_modulus, const std::vector<Seed>& seeds,
                                                  const std::vector<uint64_t>& coeffs = {}, bool host = false) {
  return shamir_shares_call(p, secrets, &pack, degree, plain_modulus, seeds, coeffs, host);
}
// dealer d shares its `pack` secrets and encrypts the shares in ONE device call (pvw_deal_shares_packed): one ciphertext per
// `pack` secrets
inline std::vector<PvwCiphertext> deal_party_shares_packed(const std::vector<uint64_t>& secrets, uint32_t pack, uint32_t degree,
                                                           uint64_t plain_modulus, const GlobalPublicKey& gpk,
                                                           const std::vector<Seed>& seeds, uint32_t out_repr = PVW_REPR_NTT) {
  return deal_call(secrets, &pack, degree, plain_modulus, gpk, &seeds, nullptr, out_repr);
}
// ... with dealer d's randomness (polynomial and encryption) from call_seed(S, c + d) of a DeviceRandomness
inline std::vector<PvwCiphertext> deal_party_shares_packed(const std::vector<uint64_t>& secrets, uint32_t pack, uint32_t degree,
                                                           uint64_t plain_modulus, const GlobalPublicKey& gpk, DeviceRandomness& rnd,
                                                           uint32_t out_repr = PVW_REPR_NTT) {
  return deal_call(secrets, &pack, degree, plain_modulus, gpk, nullptr, &rnd, out_repr);
}
// the `pack` secrets of every row, [rows][pack], from the shares [rows][indices.size()] of the parties `indices` (at least
// degree + pack of them); host only (pvw_shamir_reconstruct_packed)
inline std::vector<uint64_t> shamir_reconstruct_packed(const std::vector<uint64_t>& indices, const std::vector<uint64_t>& shares,
                                                       uint64_t plain_modulus, uint32_t pack) {
  if (indices.empty() || shares.size() % indices.size()) throw PvwError(15, "shares must hold one value per index and row");
  const size_t rows = shares.size() / indices.size();
  std::vector<uint64_t> out(rows * pack);
  check(pvw_shamir_reconstruct_packed(plain_modulus, pack, indices.data(), shares.data(), indices.size(), rows, out.data()));
  return out;
}
// the targets of shamir_evaluate_corrected that give secrets 1 .. pack-1: index p - 1 - j is the point -j
inline std::vector<uint64_t> shamir_packed_secret_indices(uint64_t plain_modulus, uint32_t pack) {
  std::vector<uint64_t> t;
  for (uint32_t j = 1; j < pack; ++j) t.push_back(plain_modulus - 1 - j);
  return t;
}
struct PackedSecrets {
  std::vector<uint64_t> secrets;    // [rows][pack]; a 0 row: undecodable
  CorrectedSecrets decode;          // what shamir_reconstruct_corrected reports for the rows (its secrets: column 0)
};
// the secrets of a packed sharing although up to (indices.size() - degree - pack) / 2 shares of each row are wrong: one
// shamir_evaluate_corrected call with polynomial degree degree + pack - 1 and the targets above (pack = 1 has none and is
// shamir_reconstruct_corrected)
inline PackedSecrets shamir_reconstruct_packed_corrected(const std::shared_ptr<PvwParameters>& p, const std::vector<uint64_t>& indices,
                                                         const std::vector<uint64_t>& shares, uint32_t degree, uint64_t plain_modulus,
                                                         uint32_t pack, bool host = false, bool party_major = false) {
  if (pack == 0) throw PvwError(1, "pack must be at least 1");
  if (pack == 1) {
    CorrectedSecrets d = shamir_reconstruct_corrected(p, indices, shares, degree, plain_modulus, host, party_major);
    std::vector<uint64_t> secrets = d.secrets;
    return PackedSecrets{std::move(secrets), std::move(d)};
  }
  EvaluatedShares e = shamir_evaluate_corrected(p, indices, shares, degree + pack - 1, plain_modulus,
                                                shamir_packed_secret_indices(plain_modulus, pack), host, party_major);
  const size_t S = e.decode.secrets.size(), K = pack;
  PackedSecrets r{std::vector<uint64_t>(S * K), std::move(e.decode)};
  for (size_t s = 0; s < S; ++s) {
    r.secrets[s * K] = r.decode.secrets[s];
    for (size_t j = 1; j < K; ++j) r.secrets[s * K + j] = e.values[s * (K - 1) + (j - 1)];
  }
  return r;
}

// the sum of the valid dealers' ciphertexts (pvw_ct_sum): same parameters and representation, no key needed
inline PvwCiphertext aggregate_ciphertexts(const std::vector<PvwCiphertext>& cts, const std::vector<bool>& valid = {}) {
  const SumInputs in = sum_inputs(cts, valid);
  const auto& p = cts[0].params;
  PvwCiphertext out{std::vector<uint64_t>(cts[0].c1.size()), std::vector<uint64_t>(cts[0].c2.size()), p, cts[0].repr};
  check(pvw_ct_sum(p->ctx, in.c1s.data(), in.c2s.data(), cts.size(), in.valid_ptr(), 0, p->n, out.c1.data(), out.c2.data(), nullptr));
  return out;
}
// party_index's aggregate share with its report (pvw_decrypt_sum_checked); bound 0 = count * noise_bound.  plain: the sum of
// the shares mod plain->modulus, or wide, where the u64 word of a field-sized sum is 0 (pvw_decrypt_sum_plain)
inline CheckedShares decrypt_party_sum(const std::vector<PvwCiphertext>& cts, const SecretKey& sk, uint32_t party_index,
                                       const std::vector<bool>& valid = {}, uint64_t bound = 0, const pvw_plain_t* plain = nullptr) {
  const SumInputs in = sum_inputs(cts, valid);
  const auto& p = cts[0].params;
  if (party_index >= p->n) throw PvwError(1, "Party index exceeds maximum");
  const size_t P = p->poly_words();
  std::vector<uint64_t> c2col;
  for (const auto& ct : cts) c2col.insert(c2col.end(), ct.c2.begin() + (size_t)party_index * P, ct.c2.begin() + (size_t)(party_index + 1) * P);
  std::vector<uint32_t> status(1);
  uint32_t count = 0;
  CheckedShares r{std::vector<uint64_t>(1), std::vector<uint64_t>(1), std::vector<bool>(1), std::vector<bool>(1)};
  if (plain_on(plain)) {
    r.wide.assign(plain->wide_words, 0);
    check(pvw_decrypt_sum_plain(p->ctx, sk.secret_coeffs.data(), in.c1s.data(), c2col.data(), cts.size(), in.valid_ptr(), cts[0].repr,
                                r.values.data(), r.noise.data(), status.data(), &count, plain->modulus, plain->wide_words, r.wide.data()));
  } else {
    check(pvw_decrypt_sum_checked(p->ctx, sk.secret_coeffs.data(), in.c1s.data(), c2col.data(), cts.size(), in.valid_ptr(), cts[0].repr,
                                  r.values.data(), r.noise.data(), status.data(), &count));
  }
  if (!bound) bound = (uint64_t)count * noise_bound(p->ctx);
  checked_report(r, status, bound, plain_on(plain));
  return r;
}
// every party's aggregate share in one call (pvw_decrypt_all_sum_checked); parties with consecutive indices
inline CheckedShares decrypt_all_party_sums(const std::vector<PvwCiphertext>& cts, const std::vector<Party>& parties,
                                            const std::vector<bool>& valid = {}, uint64_t bound = 0, const pvw_plain_t* plain = nullptr) {
  const SumInputs in = sum_inputs(cts, valid);
  const auto& p = cts[0].params;
  const size_t NP = parties.size(), kl = (size_t)p->k * p->l;
  CheckedShares r{std::vector<uint64_t>(NP), std::vector<uint64_t>(NP), std::vector<bool>(NP), std::vector<bool>(NP)};
  if (NP == 0) return r;
  std::vector<int64_t> sk(NP * kl);
  for (size_t i = 0; i < NP; ++i) {
    if (parties[i].index >= p->n || parties[i].index != parties[0].index + i) throw PvwError(1, "Party indices must be consecutive and below n");
    std::copy(parties[i].secret_key.secret_coeffs.begin(), parties[i].secret_key.secret_coeffs.end(), sk.begin() + i * kl);
  }
  std::vector<uint32_t> status(NP);
  uint32_t count = 0;
  if (plain_on(plain)) r.wide.assign(NP * plain->wide_words, 0);
  const int32_t rc =
      plain_on(plain)
          ? pvw_decrypt_all_sum_plain(p->ctx, parties[0].index, parties[0].index + (uint32_t)NP, sk.data(), in.c1s.data(), in.c2s.data(),
                                      cts.size(), in.valid_ptr(), cts[0].repr, r.values.data(), r.noise.data(), status.data(), &count,
                                      plain->modulus, plain->wide_words, r.wide.data())
          : pvw_decrypt_all_sum_checked(p->ctx, parties[0].index, parties[0].index + (uint32_t)NP, sk.data(), in.c1s.data(), in.c2s.data(),
                                        cts.size(), in.valid_ptr(), cts[0].repr, r.values.data(), r.noise.data(), status.data(), &count);
  std::fill(sk.begin(), sk.end(), 0);                                   // the copied keys do not outlive the call
  check(rc);
  if (!bound) bound = (uint64_t)count * noise_bound(p->ctx);
  checked_report(r, status, bound, plain_on(plain));
  return r;
}

// ---- weighted sums of dealers' ciphertexts ----
// the Lagrange weights at 0 of the points indices[i] + 1 mod plain_modulus, centred (pvw_shamir_lagrange_weights; host only)
inline std::vector<int64_t> shamir_lagrange_weights(const std::vector<uint64_t>& indices, uint64_t plain_modulus) {
  std::vector<int64_t> w(indices.size());
  check(pvw_shamir_lagrange_weights(plain_modulus, indices.data(), indices.size(), w.data()));
  return w;
}
// whether the combination is inside the radius the decode is PROVEN exact in (pvw_ctx_lincomb_fits; advisory)
inline bool lincomb_fits(const std::shared_ptr<PvwParameters>& p, const std::vector<int64_t>& weights, const std::vector<bool>& valid = {}) {
  if (!valid.empty() && valid.size() != weights.size()) throw PvwError(15, "valid must hold one flag per weight");
  std::vector<uint8_t> v(valid.begin(), valid.end());
  uint32_t fits = 0;
  check(pvw_ctx_lincomb_fits(p->ctx, weights.data(), weights.size(), v.empty() ? nullptr : v.data(), &fits));
  return fits != 0;
}
inline void combination_weights(const std::vector<PvwCiphertext>& cts, const std::vector<int64_t>& weights) {
  if (weights.size() != cts.size()) throw PvwError(15, "weights must hold one value per ciphertext");
}
// sum_d weights[d] cts[d] over the participating dealers (valid and weight not 0; pvw_ct_lincomb): no key needed
inline PvwCiphertext combine_ciphertexts(const std::vector<PvwCiphertext>& cts, const std::vector<int64_t>& weights,
                                         const std::vector<bool>& valid = {}) {
  const SumInputs in = sum_inputs(cts, valid);
  combination_weights(cts, weights);
  const auto& p = cts[0].params;
  PvwCiphertext out{std::vector<uint64_t>(cts[0].c1.size()), std::vector<uint64_t>(cts[0].c2.size()), p, cts[0].repr};
  check(pvw_ct_lincomb(p->ctx, in.c1s.data(), in.c2s.data(), cts.size(), in.valid_ptr(), weights.data(), 0, p->n, out.c1.data(),
                       out.c2.data(), nullptr));
  return out;
}
// The report of a combination: the noise word saturates at 2^64 - 1, so a bound of 0 means "by lincomb_fits" -- valid is that
// predicate for every entry (and not lossy, without plain options); a bound given is the noise test of the sum wrappers.
inline void combination_report(CheckedShares& r, const std::vector<uint32_t>& status, uint64_t bound, bool plain,
                               const std::shared_ptr<PvwParameters>& p, const std::vector<int64_t>& weights, const std::vector<bool>& valid) {
  checked_report(r, status, bound ? bound : ~(uint64_t)0, plain);
  if (bound) return;
  const bool fits = lincomb_fits(p, weights, valid);
  for (size_t i = 0; i < r.valid.size(); ++i) r.valid[i] = r.valid[i] && fits;
}
// party_index's share of the combination from ONE decrypt (pvw_decrypt_lincomb_plain): the new share after a handover with the
// Lagrange weights of the valid old holders and plain->modulus = p
inline CheckedShares decrypt_party_combination(const std::vector<PvwCiphertext>& cts, const std::vector<int64_t>& weights, const SecretKey& sk,
                                               uint32_t party_index, const std::vector<bool>& valid = {}, uint64_t bound = 0,
                                               const pvw_plain_t* plain = nullptr) {
  const SumInputs in = sum_inputs(cts, valid);
  combination_weights(cts, weights);
  const auto& p = cts[0].params;
  if (party_index >= p->n) throw PvwError(1, "Party index exceeds maximum");
  const size_t P = p->poly_words();
  std::vector<uint64_t> c2col;
  for (const auto& ct : cts) c2col.insert(c2col.end(), ct.c2.begin() + (size_t)party_index * P, ct.c2.begin() + (size_t)(party_index + 1) * P);
  std::vector<uint32_t> status(1);
  CheckedShares r{std::vector<uint64_t>(1), std::vector<uint64_t>(1), std::vector<bool>(1), std::vector<bool>(1)};
  if (plain_on(plain)) r.wide.assign(plain->wide_words, 0);
  check(pvw_decrypt_lincomb_plain(p->ctx, sk.secret_coeffs.data(), in.c1s.data(), c2col.data(), cts.size(), in.valid_ptr(), weights.data(),
                                  cts[0].repr, r.values.data(), r.noise.data(), status.data(), nullptr, plain_on(plain) ? plain->modulus : 0,
                                  plain_on(plain) ? plain->wide_words : 0, plain_on(plain) && plain->wide_words ? r.wide.data() : nullptr));
  combination_report(r, status, bound, plain_on(plain), p, weights, valid);
  return r;
}
// every party's share of the combination in one call (pvw_decrypt_all_lincomb_plain); parties with consecutive indices
inline CheckedShares decrypt_all_party_combinations(const std::vector<PvwCiphertext>& cts, const std::vector<int64_t>& weights,
                                                    const std::vector<Party>& parties, const std::vector<bool>& valid = {},
                                                    uint64_t bound = 0, const pvw_plain_t* plain = nullptr) {
  const SumInputs in = sum_inputs(cts, valid);
  combination_weights(cts, weights);
  const auto& p = cts[0].params;
  const size_t NP = parties.size(), kl = (size_t)p->k * p->l;
  CheckedShares r{std::vector<uint64_t>(NP), std::vector<uint64_t>(NP), std::vector<bool>(NP), std::vector<bool>(NP)};
  if (NP == 0) return r;
  std::vector<int64_t> sk(NP * kl);
  for (size_t i = 0; i < NP; ++i) {
    if (parties[i].index >= p->n || parties[i].index != parties[0].index + i) throw PvwError(1, "Party indices must be consecutive and below n");
    std::copy(parties[i].secret_key.secret_coeffs.begin(), parties[i].secret_key.secret_coeffs.end(), sk.begin() + i * kl);
  }
  std::vector<uint32_t> status(NP);
  if (plain_on(plain)) r.wide.assign(NP * plain->wide_words, 0);
  const int32_t rc = pvw_decrypt_all_lincomb_plain(
      p->ctx, parties[0].index, parties[0].index + (uint32_t)NP, sk.data(), in.c1s.data(), in.c2s.data(), cts.size(), in.valid_ptr(),
      weights.data(), cts[0].repr, r.values.data(), r.noise.data(), status.data(), nullptr, plain_on(plain) ? plain->modulus : 0,
      plain_on(plain) ? plain->wide_words : 0, plain_on(plain) && plain->wide_words ? r.wide.data() : nullptr);
  std::fill(sk.begin(), sk.end(), 0);                                   // the copied keys do not outlive the call
  check(rc);
  combination_report(r, status, bound, plain_on(plain), p, weights, valid);
  return r;
}

// ---- many combinations of the same dealers' ciphertexts ----
// row j: the Lagrange weights AT the point (targets[j] + 1) mod plain_modulus, centred (pvw_shamir_lagrange_weights_at; host only)
inline std::vector<std::vector<int64_t>> shamir_lagrange_weights_at(const std::vector<uint64_t>& indices, const std::vector<uint64_t>& targets,
                                                                    uint64_t plain_modulus) {
  std::vector<int64_t> flat(targets.size() * indices.size());
  check(pvw_shamir_lagrange_weights_at(plain_modulus, indices.data(), indices.size(), targets.data(), targets.size(), flat.data()));
  std::vector<std::vector<int64_t>> rows(targets.size());
  for (size_t j = 0; j < targets.size(); ++j) rows[j].assign(flat.begin() + j * indices.size(), flat.begin() + (j + 1) * indices.size());
  return rows;
}
// the weight rows of a packed sharing's handover: row m at the point -m (secret m), m < pack
inline std::vector<std::vector<int64_t>> shamir_packed_handover_weights(const std::vector<uint64_t>& indices, uint64_t plain_modulus, uint32_t pack) {
  std::vector<uint64_t> targets(pack);
  for (uint32_t m = 0; m < pack; ++m) targets[m] = plain_modulus - 1 - m;
  return shamir_lagrange_weights_at(indices, targets, plain_modulus);
}
// weight_rows [R][D] flattened row-major
inline std::vector<int64_t> combination_weight_rows(const std::vector<PvwCiphertext>& cts, const std::vector<std::vector<int64_t>>& weight_rows) {
  if (weight_rows.empty()) throw PvwError(1, "num_combos must be at least 1");
  std::vector<int64_t> flat;
  for (const auto& row : weight_rows) {
    combination_weights(cts, row);
    flat.insert(flat.end(), row.begin(), row.end());
  }
  return flat;
}
// element r = combine_ciphertexts(cts, weight_rows[r], valid), every ciphertext read once per tile of rows (pvw_ct_lincomb_many)
inline std::vector<PvwCiphertext> combine_ciphertexts_many(const std::vector<PvwCiphertext>& cts, const std::vector<std::vector<int64_t>>& weight_rows,
                                                           const std::vector<bool>& valid = {}) {
  const SumInputs in = sum_inputs(cts, valid);
  const std::vector<int64_t> w = combination_weight_rows(cts, weight_rows);
  const auto& p = cts[0].params;
  const size_t R = weight_rows.size(), n1 = cts[0].c1.size(), n2 = cts[0].c2.size();
  std::vector<uint64_t> c1(R * n1), c2(R * n2);
  check(pvw_ct_lincomb_many(p->ctx, in.c1s.data(), in.c2s.data(), cts.size(), in.valid_ptr(), w.data(), R, 0, p->n, c1.data(), c2.data(), nullptr));
  std::vector<PvwCiphertext> out;
  for (size_t r = 0; r < R; ++r)
    out.push_back(PvwCiphertext{std::vector<uint64_t>(c1.begin() + r * n1, c1.begin() + (r + 1) * n1),
                                std::vector<uint64_t>(c2.begin() + r * n2, c2.begin() + (r + 1) * n2), p, cts[0].repr});
  return out;
}
// every party's share of every combination in one call (pvw_decrypt_all_lincomb_many_plain): arrays [parties][R]; the report's
// valid follows combination_report row by row
inline CheckedShares decrypt_all_party_combinations_many(const std::vector<PvwCiphertext>& cts, const std::vector<std::vector<int64_t>>& weight_rows,
                                                         const std::vector<Party>& parties, const std::vector<bool>& valid = {},
                                                         uint64_t bound = 0, const pvw_plain_t* plain = nullptr) {
  const SumInputs in = sum_inputs(cts, valid);
  const std::vector<int64_t> w = combination_weight_rows(cts, weight_rows);
  const auto& p = cts[0].params;
  const size_t NP = parties.size(), R = weight_rows.size(), kl = (size_t)p->k * p->l;
  CheckedShares r{std::vector<uint64_t>(NP * R), std::vector<uint64_t>(NP * R), std::vector<bool>(NP * R), std::vector<bool>(NP * R)};
  if (NP == 0) return r;
  std::vector<int64_t> sk(NP * kl);
  for (size_t i = 0; i < NP; ++i) {
    if (parties[i].index >= p->n || parties[i].index != parties[0].index + i) throw PvwError(1, "Party indices must be consecutive and below n");
    std::copy(parties[i].secret_key.secret_coeffs.begin(), parties[i].secret_key.secret_coeffs.end(), sk.begin() + i * kl);
  }
  std::vector<uint32_t> status(NP * R);
  if (plain_on(plain)) r.wide.assign(NP * R * plain->wide_words, 0);
  const int32_t rc = pvw_decrypt_all_lincomb_many_plain(
      p->ctx, parties[0].index, parties[0].index + (uint32_t)NP, sk.data(), in.c1s.data(), in.c2s.data(), cts.size(), in.valid_ptr(), w.data(), R,
      cts[0].repr, r.values.data(), r.noise.data(), status.data(), nullptr, plain_on(plain) ? plain->modulus : 0,
      plain_on(plain) ? plain->wide_words : 0, plain_on(plain) && plain->wide_words ? r.wide.data() : nullptr);
  std::fill(sk.begin(), sk.end(), 0);                                   // the copied keys do not outlive the call
  check(rc);
  checked_report(r, status, bound ? bound : ~(uint64_t)0, plain_on(plain));
  if (bound) return r;
  for (size_t c = 0; c < R; ++c) {
    const bool fits = lincomb_fits(p, weight_rows[c], valid);
    for (size_t i = 0; i < NP; ++i) r.valid[i * R + c] = r.valid[i * R + c] && fits;
  }
  return r;
}

// ---- Handover over a prime below 2^256: the weight rows of signed digits, the fold of the digit plaintexts and the
// call that ties them to one many-combinations pass.  The public pieces run on the host cores (the *_host entry points); the
// device forms take device pointers and are reached through the C ABI.
struct WideHandoverShape {
  uint32_t num_limbs, num_digits;
};
inline WideHandoverShape shamir_wide_handover_shape(const Wide& plain_modulus, uint32_t limb_bits = 52, uint32_t digit_bits = 64) {
  WideHandoverShape s{0, 0};
  check(pvw_shamir_wide_handover_shape(plain_modulus.data(), limb_bits, digit_bits, &s.num_limbs, &s.num_digits));
  return s;
}
// digits [count][V] of values [count][4] (pvw_shamir_wide_signed_digits_host)
inline std::vector<int64_t> shamir_wide_signed_digits(const std::vector<uint64_t>& values, const Wide& plain_modulus, uint32_t digit_bits = 64) {
  if (values.size() % PVW_WIDE_WORDS) throw PvwError(15, "four words per value");
  const size_t count = values.size() / PVW_WIDE_WORDS;
  std::vector<int64_t> out(count * shamir_wide_handover_shape(plain_modulus, 62, digit_bits).num_digits);
  check(pvw_shamir_wide_signed_digits_host(plain_modulus.data(), values.data(), count, digit_bits, out.data()));
  return out;
}
// the points 0, -1, .., -(pack-1) of a packed wide sharing as field elements [pack][4] (-m is p - m)
inline std::vector<uint64_t> shamir_packed_wide_handover_points(const Wide& plain_modulus, uint32_t pack) {
  std::vector<uint64_t> out((size_t)pack * PVW_WIDE_WORDS, 0);
  for (uint32_t m = 1; m < pack; ++m) {
    uint64_t br = m;
    for (int i = 0; i < PVW_WIDE_WORDS; ++i) {
      const uint64_t v = plain_modulus[i];
      out[(size_t)m * PVW_WIDE_WORDS + i] = v - br;
      br = v < br;
    }
  }
  return out;
}
// weight rows [T V][D NL] (pvw_shamir_wide_handover_weights_host); points [T][4], empty = the single point 0
inline std::vector<int64_t> shamir_wide_handover_weights(const std::vector<uint64_t>& indices, const Wide& plain_modulus,
                                                         const std::vector<bool>& valid = {}, const std::vector<uint64_t>& points = {},
                                                         uint32_t limb_bits = 52, uint32_t digit_bits = 64) {
  if (!valid.empty() && valid.size() != indices.size()) throw PvwError(15, "valid must hold one flag per holder");
  if (points.size() % PVW_WIDE_WORDS) throw PvwError(15, "four words per point");
  const std::vector<uint8_t> v(valid.begin(), valid.end());
  const size_t T = points.empty() ? 1 : points.size() / PVW_WIDE_WORDS;
  const WideHandoverShape s = shamir_wide_handover_shape(plain_modulus, limb_bits, digit_bits);
  std::vector<int64_t> out(T * s.num_digits * indices.size() * s.num_limbs);
  check(pvw_shamir_wide_handover_weights_host(plain_modulus.data(), indices.data(), v.empty() ? nullptr : v.data(), indices.size(),
                                              points.empty() ? nullptr : points.data(), T, limb_bits, digit_bits, out.data()));
  return out;
}
struct WideHandoverShares {
  std::vector<uint64_t> values;     // [count][4], fully reduced
  std::vector<uint32_t> status;     // [count]: the OR of the digit decodes' status words without PVW_DEC_NEGATIVE
  uint32_t count = 0;               // the valid holders (decrypt_all_party_handover_wide)
};
// values[i] = sum_v +-wide[i][v] 2^(digit_bits v) mod p from wide [count][V][wide_words], status [count][V]
// (pvw_shamir_wide_from_digits_host)
inline WideHandoverShares shamir_wide_from_digits(const std::vector<uint64_t>& wide, const std::vector<uint32_t>& status, uint32_t num_digits,
                                                  uint32_t wide_words, const Wide& plain_modulus, uint32_t digit_bits = 64) {
  if (num_digits == 0 || wide_words == 0 || status.size() % num_digits || wide.size() != status.size() * wide_words)
    throw PvwError(15, "wide must hold wide_words words per status word, num_digits of them per element");
  const size_t count = status.size() / num_digits;
  WideHandoverShares r{std::vector<uint64_t>(count * PVW_WIDE_WORDS), std::vector<uint32_t>(count), 0};
  std::vector<uint32_t> st(status);
  check(pvw_shamir_wide_from_digits_host(plain_modulus.data(), digit_bits, num_digits, wide.data(), st.data(), wide_words, count, r.values.data(),
                                         r.status.data()));
  return r;
}
// whether every weight row of a wide handover is inside the radius the decode is PROVEN exact in (pvw_ctx_wide_handover_fits)
inline bool wide_handover_fits(const std::shared_ptr<PvwParameters>& p, const Wide& plain_modulus, size_t num_valid, uint32_t limb_bits = 52,
                               uint32_t digit_bits = 64) {
  uint32_t fits = 0;
  check(pvw_ctx_wide_handover_fits(p->ctx, plain_modulus.data(), num_valid, limb_bits, digit_bits, &fits));
  return fits != 0;
}
// every new party's new share in one call (pvw_decrypt_all_handover_wide): cts holds the old holders' limb ciphertexts, vector
// d NL + w limb w of holder d; values [parties][T][4]
inline WideHandoverShares decrypt_all_party_handover_wide(const std::vector<PvwCiphertext>& cts, const std::vector<Party>& parties,
                                                          const std::vector<uint64_t>& indices, const Wide& plain_modulus,
                                                          const std::vector<bool>& valid = {}, const std::vector<uint64_t>& points = {},
                                                          uint32_t limb_bits = 52, uint32_t digit_bits = 64) {
  const SumInputs in = sum_inputs(cts, {});
  const auto& p = cts[0].params;
  const uint32_t NL = shamir_wide_limbs(plain_modulus, limb_bits);
  if (indices.empty() || cts.size() != indices.size() * NL) throw PvwError(15, "num_limbs ciphertexts per holder");
  if (!valid.empty() && valid.size() != indices.size()) throw PvwError(15, "valid must hold one flag per holder");
  if (points.size() % PVW_WIDE_WORDS) throw PvwError(15, "four words per point");
  const std::vector<uint8_t> v(valid.begin(), valid.end());
  const size_t NP = parties.size(), T = points.empty() ? 1 : points.size() / PVW_WIDE_WORDS, kl = (size_t)p->k * p->l;
  WideHandoverShares r{std::vector<uint64_t>(NP * T * PVW_WIDE_WORDS), std::vector<uint32_t>(NP * T), 0};
  if (NP == 0) return r;
  std::vector<int64_t> sk(NP * kl);
  for (size_t i = 0; i < NP; ++i) {
    if (parties[i].index >= p->n || parties[i].index != parties[0].index + i) throw PvwError(1, "Party indices must be consecutive and below n");
    std::copy(parties[i].secret_key.secret_coeffs.begin(), parties[i].secret_key.secret_coeffs.end(), sk.begin() + i * kl);
  }
  const int32_t rc = pvw_decrypt_all_handover_wide(p->ctx, parties[0].index, parties[0].index + (uint32_t)NP, sk.data(), in.c1s.data(),
                                                   in.c2s.data(), indices.size(), plain_modulus.data(), limb_bits, digit_bits, indices.data(),
                                                   v.empty() ? nullptr : v.data(), points.empty() ? nullptr : points.data(), T, cts[0].repr,
                                                   r.values.data(), r.status.data(), &r.count);
  std::fill(sk.begin(), sk.end(), 0);                                   // the copied keys do not outlive the call
  check(rc);
  return r;
}

// ---- The one-word handover from a mask.  The host forms; the device forms take device pointers (the mask among
// them) and are reached through the C ABI.
struct HandoverWeights {
  std::vector<int64_t> weights;     // [T][D], row-major; a masked holder's column is 0
  uint32_t count = 0;               // the valid holders
};
// row j = the Lagrange weights AT (targets[j] + 1) mod p over the valid holders (pvw_shamir_handover_weights_host); targets empty =
// the single point 0
inline HandoverWeights shamir_handover_weights(const std::vector<uint64_t>& indices, uint64_t plain_modulus, const std::vector<bool>& valid = {},
                                               const std::vector<uint64_t>& targets = {}) {
  if (!valid.empty() && valid.size() != indices.size()) throw PvwError(15, "valid must hold one flag per holder");
  const std::vector<uint8_t> v(valid.begin(), valid.end());
  const size_t T = targets.empty() ? 1 : targets.size();
  HandoverWeights r{std::vector<int64_t>(T * indices.size()), 0};
  check(pvw_shamir_handover_weights_host(plain_modulus, indices.data(), v.empty() ? nullptr : v.data(), indices.size(),
                                         targets.empty() ? nullptr : targets.data(), T, r.weights.data(), &r.count));
  return r;
}
struct ValidMask {
  std::vector<uint8_t> valid;       // [count]
  uint32_t num_valid = 0;
};
// valid[c] = 1 iff no row of the [rows][count] report has status & status_bits or noise > noise_bound in column c
// (pvw_shamir_valid_mask_host); either array may be empty, not both
inline ValidMask shamir_valid_mask(const std::vector<uint32_t>& status, const std::vector<uint64_t>& noise, size_t count,
                                   uint32_t status_bits = 0xFFFFFFFFu, uint64_t noise_bound = ~(uint64_t)0) {
  const size_t have = status.empty() ? noise.size() : status.size();
  if (count == 0 || have % count || (!status.empty() && !noise.empty() && status.size() != noise.size()))
    throw PvwError(15, "status and noise must be [rows][count] arrays of one shape");
  std::vector<uint32_t> st(status);
  ValidMask r{std::vector<uint8_t>(count), 0};
  check(pvw_shamir_valid_mask_host(st.empty() ? nullptr : st.data(), noise.empty() ? nullptr : noise.data(), status_bits, noise_bound, count,
                                   have / count, count, 1, r.valid.data(), &r.num_valid));
  return r;
}
// every new party's new share in one call (pvw_decrypt_all_handover): cts holds the old holders' re-dealt ciphertexts, holder d at
// party index indices[d]; arrays [parties][T]; .count of the result is the number of valid holders
struct HandoverShares : CheckedShares {
  uint32_t count = 0;
};
inline HandoverShares decrypt_all_party_handover(const std::vector<PvwCiphertext>& cts, const std::vector<Party>& parties,
                                                 const std::vector<uint64_t>& indices, uint64_t plain_modulus,
                                                 const std::vector<bool>& valid = {}, const std::vector<uint64_t>& targets = {},
                                                 uint64_t bound = 0, uint32_t wide_words = 0) {
  const SumInputs in = sum_inputs(cts, {});
  const auto& p = cts[0].params;
  if (cts.size() != indices.size()) throw PvwError(15, "one ciphertext per holder");
  if (!valid.empty() && valid.size() != indices.size()) throw PvwError(15, "valid must hold one flag per holder");
  const std::vector<uint8_t> v(valid.begin(), valid.end());
  const size_t NP = parties.size(), T = targets.empty() ? 1 : targets.size(), kl = (size_t)p->k * p->l;
  HandoverShares r;
  r.values.assign(NP * T, 0), r.noise.assign(NP * T, 0), r.lossy.assign(NP * T, false), r.valid.assign(NP * T, false);
  if (NP == 0) return r;
  std::vector<int64_t> sk(NP * kl);
  for (size_t i = 0; i < NP; ++i) {
    if (parties[i].index >= p->n || parties[i].index != parties[0].index + i) throw PvwError(1, "Party indices must be consecutive and below n");
    std::copy(parties[i].secret_key.secret_coeffs.begin(), parties[i].secret_key.secret_coeffs.end(), sk.begin() + i * kl);
  }
  std::vector<uint32_t> status(NP * T);
  if (wide_words) r.wide.assign(NP * T * wide_words, 0);
  const int32_t rc = pvw_decrypt_all_handover(p->ctx, parties[0].index, parties[0].index + (uint32_t)NP, sk.data(), in.c1s.data(), in.c2s.data(),
                                              indices.size(), v.empty() ? nullptr : v.data(), indices.data(),
                                              targets.empty() ? nullptr : targets.data(), T, cts[0].repr, r.values.data(), r.noise.data(),
                                              status.data(), &r.count, plain_modulus, wide_words, wide_words ? r.wide.data() : nullptr);
  std::fill(sk.begin(), sk.end(), 0);                                   // the copied keys do not outlive the call
  check(rc);
  checked_report(r, status, bound ? bound : ~(uint64_t)0, true);
  return r;
}

}  // namespace pvw_host

// Key generation from a seed through the C++ mirror: GlobalPublicKey::generate_all_party_keys(lo, hi, sk_seed, seed)
// (pvw_keygen_seeded) gives the public key that Party::create + generate_all_party_keys(parties, seed) gives, byte for byte,
// and ciphertexts under it decrypt with SecretKey::random(sk_seed, i) -- generate_all_party_keys over Party::new
// (public_key.rs:376-401, :62-79) without the keys on the host.
// `host`: the refusals that need no GPU.  Built by tests/test_keygen_seeded_host.py everywhere; run in full on the GPU box.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

template <class F>
static bool refused(F&& f, int32_t code, const char* text) {
  try {
    f();
  } catch (const PvwError& e) {
    return e.code == code && std::strstr(e.what(), text) != nullptr;
  }
  return false;
}

int main(int argc, char** argv) {
  try {
    const bool host_only = argc > 1 && std::strcmp(argv[1], "host") == 0;
    const std::vector<uint64_t> moduli = {0xffffee001ULL, 0xffffc4001ULL, 0x1ffffe0001ULL};
    const uint32_t n = 70, k = 9, l = 8;
    auto [bound1, bound2] = PvwParameters::suggest_error_bounds(n, k, l, moduli, 0.5f);
    auto params = PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
                      .set_secret_variance(0.5f).set_error_bounds_u32(bound1, bound2).build_arc();
    Seed sk_seed, seed;
    sk_seed.fill(0x3D);
    seed.fill(0x5C);
    // the argument checks come before any device work
    PvwCrs none{params};
    GlobalPublicKey empty(none);
    if (!refused([&] { empty.generate_all_party_keys(5, 3, sk_seed, seed); }, 1, "party_lo > party_hi")) { printf("range not refused\n"); return 1; }
    if (!refused([&] { empty.generate_all_party_keys(0, n + 1, sk_seed, seed); }, 1, "exceeds maximum")) { printf("party_hi not refused\n"); return 1; }
    if (!refused([&] { sample_secret_keys_device(params, sk_seed, 0, 1, nullptr); }, 1, "NULL argument")) { printf("NULL buffer not refused\n"); return 1; }
    if (host_only) {
      printf("KEYGEN_SEEDED_CPP_HOST_OK\n");
      return 0;
    }
    PvwCrs crs = PvwCrs::new_deterministic(params, seed);
    GlobalPublicKey drawn(crs);
    drawn.generate_all_party_keys(0, n, sk_seed, seed);
    const std::vector<uint8_t> b_drawn = drawn.to_bytes(0, n, PVW_REPR_NTT);
    std::vector<Party> parties;
    for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, sk_seed));
    GlobalPublicKey classic(crs);
    classic.generate_all_party_keys(parties, seed);
    if (b_drawn != classic.to_bytes(0, n, PVW_REPR_NTT)) { printf("the seeded public key differs from the two-step one\n"); return 1; }
    // a sub-range over the classic key rewrites the same rows
    classic.generate_all_party_keys(37, n, sk_seed, seed);
    if (b_drawn != classic.to_bytes(0, n, PVW_REPR_NTT)) { printf("the seeded sub-range differs\n"); return 1; }
    if (classic.num_public_keys() != n || !classic.is_full()) { printf("key count\n"); return 1; }
    drawn.generate_all_party_keys(0, n, sk_seed, seed);
    std::vector<uint64_t> scalars;
    for (uint32_t i = 0; i < n; ++i) scalars.push_back(i * 1000 + 1);
    PvwCiphertext ct = encrypt(scalars, drawn, seed);
    uint32_t correct = 0;
    for (uint32_t i = 0; i < n; ++i) correct += decrypt_party_value(ct, SecretKey::random(params, sk_seed, i), i) == scalars[i];
    if (correct < n * 95 / 100) { printf("only %u of %u scalars recovered\n", correct, n); return 1; }
    // the resident key drawn on the device is a handle like any other
    { DeviceSecretKey resident(params, sk_seed, 3); if (!resident.raw()) { printf("no resident key\n"); return 1; } }
    printf("KEYGEN_SEEDED_CPP_OK %u/%u\n", correct, n);
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

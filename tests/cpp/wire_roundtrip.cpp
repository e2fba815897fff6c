// Wire format v1 through the C++ mirror (pvw_host::PvwCiphertext / GlobalPublicKey ::to_bytes / ::from_bytes): ciphertexts and
// the public key written in one context, read in a second context with the same parameters, decrypt to the dealt values.
// Built and run by tests/test_gpu_wire.py.
#include <cstdio>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

int main() {
  try {
    const std::vector<uint64_t> moduli = {0xffffee001ULL, 0xffffc4001ULL, 0x1ffffe0001ULL};
    const uint32_t n = 12;
    auto [bound1, bound2] = PvwParameters::suggest_error_bounds(n, 4, 16, moduli, 0.5f);
    auto make = [&]() {
      return PvwParametersBuilder().set_parties(n).set_dimension(4).set_l(16).set_moduli(moduli).set_secret_variance(0.5f)
          .set_error_bounds_u32(bound1, bound2).build_arc();
    };
    auto pa = make(), pb = make();
    Seed seed;
    seed.fill(0x3D);
    PvwCrs crs_a = PvwCrs::new_deterministic(pa, seed), crs_b = PvwCrs::new_deterministic(pb, seed);
    GlobalPublicKey gpk(crs_a);
    std::vector<Party> parties;
    for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, pa, seed));
    gpk.generate_all_party_keys(parties, seed);
    // the key moves as bytes; the second context encrypts with it
    GlobalPublicKey gpk_b = GlobalPublicKey::from_bytes(crs_b, gpk.to_bytes(0, n));
    if (gpk_b.num_public_keys() != n) { printf("num_public_keys %u\n", gpk_b.num_public_keys()); return 1; }
    std::vector<std::vector<uint64_t>> all(n);
    for (uint32_t d = 0; d < n; ++d)
      for (uint32_t j = 0; j < n; ++j) all[d].push_back(d * 100 + j + 7);
    auto cts = encrypt_all_party_shares(all, gpk_b, seed);
    std::vector<PvwCiphertext> back;
    for (const auto& ct : cts) {
      auto blob = ct.to_bytes();
      back.push_back(PvwCiphertext::from_bytes(pa, blob));
      if (back.back().c1 != ct.c1 || back.back().c2 != ct.c2) { printf("ciphertext round trip differs\n"); return 1; }
    }
    auto res = decrypt_all_party_shares(back, parties);
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t d = 0; d < n; ++d)
        if (res[i][d] != all[d][i]) { printf("party %u dealer %u: %llu\n", i, d, (unsigned long long)res[i][d]); return 1; }
    // a corrupted blob is refused
    auto blob = cts[0].to_bytes();
    for (size_t i = blob.size() - 8; i < blob.size(); ++i) blob[i] = 0xFF;
    try {
      PvwCiphertext::from_bytes(pa, blob);
      printf("corrupted blob accepted\n");
      return 1;
    } catch (const PvwError& e) {
      if (e.code != PVW_ERR_DESERIALIZATION) { printf("wrong error: %s\n", e.what()); return 1; }
    }
    printf("WIRE_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

// Encrypt from a device randomness state through the C++ mirror (pvw_host::DeviceRandomness): call_seed against fixed
// words everywhere; with a device, an encrypt and a multi-dealer encrypt against the seed-mode calls under the derived seeds.
// Built and run by tests/test_device_randomness_host.py.
#include <cstdio>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

int main() {
  try {
    Seed s{};
    for (int i = 0; i < 32; ++i) s[i] = (uint8_t)i;
    // words 0..7 of ChaCha8(key = 00 01 .. 1f, block counter 5, stream (8 << 32) | 0), little-endian
    const uint8_t want5[32] = {0x07, 0xf4, 0x49, 0x7d, 0x0a, 0x3a, 0x36, 0x0a, 0x26, 0x4b, 0x61, 0x42, 0xb6, 0x04, 0xe7, 0x4b,
                               0x27, 0x13, 0x8c, 0xa0, 0xee, 0xa4, 0x7c, 0xa7, 0x22, 0x52, 0x62, 0xb7, 0x3a, 0xed, 0xf1, 0x5f};
    const Seed got = DeviceRandomness::call_seed(s, 5);
    for (int i = 0; i < 32; ++i)
      if (got[i] != want5[i]) { printf("call_seed byte %d differs\n", i); return 1; }
    printf("call_seed ok\n");
    if (!pvw_device_available()) return 0;
    const std::vector<uint64_t> moduli = {0xffffee001ULL, 0xffffc4001ULL, 0x1ffffe0001ULL};
    const uint32_t n = 12;
    auto [bound1, bound2] = PvwParameters::suggest_error_bounds(n, 8, 8, moduli, 0.5f);
    auto params = PvwParametersBuilder().set_parties(n).set_dimension(8).set_l(8).set_moduli(moduli)
                      .set_secret_variance(0.5f).set_error_bounds_u32(bound1, bound2).build_arc();
    PvwCrs crs = PvwCrs::new_deterministic(params, s);
    GlobalPublicKey gpk(crs);
    std::vector<Party> parties;
    for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, s));
    gpk.generate_all_party_keys(parties, s);
    DeviceRandomness rnd(params, s, 40);
    std::vector<uint64_t> m(n);
    for (uint32_t j = 0; j < n; ++j) m[j] = 7 * j + 3;
    const PvwCiphertext a = encrypt(m, gpk, rnd), b = encrypt(m, gpk, DeviceRandomness::call_seed(s, 40));
    if (a.c1 != b.c1 || a.c2 != b.c2 || rnd.counter() != 41) { printf("encrypt from the state differs\n"); return 1; }
    std::vector<std::vector<uint64_t>> all(n, m);
    const auto cts = encrypt_all_party_shares(all, gpk, rnd);
    for (uint32_t d = 0; d < n; ++d) {
      const PvwCiphertext w = encrypt(m, gpk, DeviceRandomness::call_seed(s, 41 + d));
      if (cts[d].c1 != w.c1 || cts[d].c2 != w.c2) { printf("dealer %u differs\n", d); return 1; }
    }
    if (rnd.counter() != 41 + n) { printf("counter %llu\n", (unsigned long long)rnd.counter()); return 1; }
    if (decrypt_party_value(cts[3], parties[5].secret_key, 5) != m[5]) { printf("decrypt failed\n"); return 1; }
    DeviceRandomness fresh(params);   // seeded from the OS
    (void)encrypt(m, gpk, fresh);
    printf("DEVICE_RANDOMNESS_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

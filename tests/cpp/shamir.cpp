// Shamir shares through the C++ mirror (pvw_host::shamir_shares, deal_party_shares, shamir_reconstruct).
// "host": the restatement and the reconstruction, no GPU.  No argument: the whole loop on the device -- secrets -> ciphertexts ->
// aggregated ciphertext -> each party's aggregate share mod p -> the sum of the valid dealers' secrets.
// Built by tests/test_shamir_host.py everywhere; the device half is run by tests/test_gpu_shamir.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

static const uint64_t P61 = (1ULL << 61) - 1;

static std::vector<Seed> make_seeds(size_t D) {
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x51 + d));
  return seeds;
}

static int host_half() {
  const uint32_t n = 12, t = 4;
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const std::vector<uint64_t> secrets = {5, ~0ULL, P61 + 3};
  const size_t D = secrets.size();
  const std::vector<uint64_t> shares = shamir_shares(params, secrets, t, P61, make_seeds(D), {}, true);
  const std::vector<uint64_t> idx = {11, 0, 7, 3, 5};
  std::vector<uint64_t> picked;
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.push_back(shares[d * n + i]);
  const std::vector<uint64_t> back = shamir_reconstruct(idx, picked, P61);
  for (size_t d = 0; d < D; ++d)
    if (back[d] != secrets[d] % P61) {
      printf("dealer %zu: %llu, expected %llu\n", d, (unsigned long long)back[d], (unsigned long long)(secrets[d] % P61));
      return 1;
    }
  // explicit coefficients: f(x) = 9 + 2 x + x^2
  const std::vector<uint64_t> ex = shamir_shares(params, {9}, 2, 65537, {}, {2, 1}, true);
  for (uint32_t i = 0; i < n; ++i)
    if (ex[i] != 9 + 2 * (i + 1) + (uint64_t)(i + 1) * (i + 1)) return 1;
  bool refused = false;
  try {
    shamir_shares(params, secrets, t, 561, make_seeds(D), {}, true);
  } catch (const PvwError&) {
    refused = true;
  }
  if (!refused) return 1;
  printf("SHAMIR_CPP_HOST_OK\n");
  return 0;
}

static int device_half() {
  const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
  const uint32_t n = 8, t = 3;
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(4).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  Seed seed;
  seed.fill(0x3D);
  PvwCrs crs = PvwCrs::new_deterministic(params, seed);
  GlobalPublicKey global_pk(crs);
  std::vector<Party> parties;
  for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, seed));
  global_pk.generate_all_party_keys(parties, seed);
  const size_t D = 6;
  std::vector<uint64_t> secrets;
  for (size_t d = 0; d < D; ++d) secrets.push_back(P61 - 1 - d);
  const std::vector<Seed> seeds = make_seeds(D);
  if (shamir_shares(params, secrets, t, P61, seeds) != shamir_shares(params, secrets, t, P61, seeds, {}, true)) {
    printf("device shares differ from the host's\n");
    return 1;
  }
  auto cts = deal_party_shares(secrets, t, P61, global_pk, seeds);
  const std::vector<bool> valid = {true, false, true, true, true, true};
  const pvw_plain_t plain{P61, 0, nullptr};
  CheckedShares sums = decrypt_all_party_sums(cts, parties, valid, 0, &plain);
  uint64_t want = 0;
  for (size_t d = 0; d < D; ++d)
    if (valid[d]) want = (want + secrets[d]) % P61;
  const std::vector<uint64_t> idx = {6, 1, 4, 3};
  std::vector<uint64_t> picked;
  for (uint64_t i : idx) picked.push_back(sums.values[i]);
  const uint64_t got = shamir_reconstruct(idx, picked, P61)[0];
  if (got != want) {
    printf("reconstructed %llu, expected %llu\n", (unsigned long long)got, (unsigned long long)want);
    return 1;
  }
  printf("SHAMIR_CPP_OK\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    return argc > 1 && !strcmp(argv[1], "host") ? host_half() : device_half();
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

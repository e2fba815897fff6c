// Packed Shamir sharing through the C++ mirror (pvw_host::shamir_shares_packed, deal_party_shares_packed,
// shamir_reconstruct_packed, shamir_reconstruct_packed_corrected).
// "host": the restatement and both reconstructions, no GPU.  No argument: the whole loop on the device -- secrets [D][K] ->
// D ciphertexts -> aggregated ciphertext -> each party's aggregate share mod p -> the K sums of the valid dealers' secrets.
// Built by tests/test_shamir_packed_host.py everywhere; the device half is run by tests/test_gpu_shamir_packed.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

static const uint64_t P61 = (1ULL << 61) - 1;

static std::vector<Seed> make_seeds(size_t D) {
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x61 + d));
  return seeds;
}

static int host_half() {
  const uint32_t n = 12, K = 3, t = 4;
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const std::vector<uint64_t> secrets = {5, ~0ULL, P61 + 3, 0, P61 - 1, 77};   // [2][3]
  const size_t D = secrets.size() / K;
  const std::vector<uint64_t> shares = shamir_shares_packed(params, secrets, K, t, P61, make_seeds(D), {}, true);
  const std::vector<uint64_t> idx = {11, 0, 7, 3, 5, 9, 2};                     // t + K parties
  std::vector<uint64_t> picked;
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.push_back(shares[d * n + i]);
  const std::vector<uint64_t> back = shamir_reconstruct_packed(idx, picked, P61, K);
  for (size_t e = 0; e < secrets.size(); ++e)
    if (back[e] != secrets[e] % P61) {
      printf("secret %zu: %llu, expected %llu\n", e, (unsigned long long)back[e], (unsigned long long)(secrets[e] % P61));
      return 1;
    }
  // pack = 1 is the unpacked sharing, word for word
  const std::vector<uint64_t> one = {5, ~0ULL, P61 + 3};
  if (shamir_shares_packed(params, one, 1, t, P61, make_seeds(3), {}, true) != shamir_shares(params, one, t, P61, make_seeds(3), {}, true)) {
    printf("pack = 1 differs from shamir_shares\n");
    return 1;
  }
  // all n shares, two of each row wrong: (12 - 4 - 3) / 2 = 2 are corrected
  std::vector<uint64_t> idx_all, noisy = shares;
  for (uint32_t i = 0; i < n; ++i) idx_all.push_back(i);
  noisy[1] ^= 1, noisy[8] += 5, noisy[n + 0] += 1, noisy[n + 11] ^= 4;
  const PackedSecrets fixed = shamir_reconstruct_packed_corrected(nullptr, idx_all, noisy, t, P61, K, true);
  for (size_t e = 0; e < secrets.size(); ++e)
    if (fixed.secrets[e] != secrets[e] % P61) {
      printf("corrected secret %zu: %llu\n", e, (unsigned long long)fixed.secrets[e]);
      return 1;
    }
  if (fixed.decode.nerr[0] != 2 || fixed.decode.nerr[1] != 2 || !fixed.decode.wrong(0, 8) || !fixed.decode.wrong(1, 11)) return 1;
  // pack = 1 is the corrected reconstruction of an ordinary sharing: (12 - 4 - 1) / 2 = 3 wrong shares
  std::vector<uint64_t> plain = shamir_shares(params, one, t, P61, make_seeds(3), {}, true);
  plain[2] += 1, plain[5] ^= 2, plain[10] += 7, plain[n + 4] += 3;
  const PackedSecrets p1 = shamir_reconstruct_packed_corrected(nullptr, idx_all, plain, t, P61, 1, true);
  const CorrectedSecrets c1 = shamir_reconstruct_corrected(nullptr, idx_all, plain, t, P61, true);
  if (p1.secrets != c1.secrets || p1.decode.nerr != c1.nerr || p1.decode.err_mask != c1.err_mask || p1.decode.nerr[0] != 3) return 1;
  for (size_t d = 0; d < 3; ++d)
    if (p1.secrets[d] != one[d] % P61) return 1;
  bool refused = false;
  try {
    shamir_shares_packed(params, secrets, K, n - K + 1, P61, make_seeds(D), {}, true);   // degree + pack > n
  } catch (const PvwError&) {
    refused = true;
  }
  if (!refused) return 1;
  printf("SHAMIR_PACKED_CPP_HOST_OK\n");
  return 0;
}

static int device_half() {
  const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
  const uint32_t n = 8, K = 3, t = 2;
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
  for (size_t e = 0; e < D * K; ++e) secrets.push_back(P61 - 1 - 3 * e);
  const std::vector<Seed> seeds = make_seeds(D);
  if (shamir_shares_packed(params, secrets, K, t, P61, seeds) != shamir_shares_packed(params, secrets, K, t, P61, seeds, {}, true)) {
    printf("device shares differ from the host's\n");
    return 1;
  }
  auto cts = deal_party_shares_packed(secrets, K, t, P61, global_pk, seeds);
  const std::vector<bool> valid = {true, false, true, true, true, true};
  const pvw_plain_t plain{P61, 0, nullptr};
  CheckedShares sums = decrypt_all_party_sums(cts, parties, valid, 0, &plain);
  std::vector<uint64_t> want(K, 0);
  for (size_t d = 0; d < D; ++d)
    if (valid[d])
      for (uint32_t j = 0; j < K; ++j) want[j] = (want[j] + secrets[d * K + j] % P61) % P61;
  const std::vector<uint64_t> idx = {6, 1, 4, 3, 0};                            // t + K parties
  std::vector<uint64_t> picked;
  for (uint64_t i : idx) picked.push_back(sums.values[i]);
  if (shamir_reconstruct_packed(idx, picked, P61, K) != want) {
    printf("reconstructed sums differ\n");
    return 1;
  }
  // all 8 parties' sums, one of them wrong: (8 - 2 - 3) / 2 = 1 is corrected, on the device
  std::vector<uint64_t> idx_all, all = sums.values;
  for (uint32_t i = 0; i < n; ++i) idx_all.push_back(i);
  all[5] ^= 9;
  const PackedSecrets fixed = shamir_reconstruct_packed_corrected(params, idx_all, all, t, P61, K);
  if (fixed.secrets != want || fixed.decode.nerr[0] != 1 || !fixed.decode.wrong(0, 5)) {
    printf("corrected sums differ\n");
    return 1;
  }
  printf("SHAMIR_PACKED_CPP_OK\n");
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

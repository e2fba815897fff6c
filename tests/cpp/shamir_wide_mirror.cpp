// Shamir shares over a 256-bit prime field through the C++ mirror (pvw_host::shamir_shares_wide, deal_party_shares_wide,
// shamir_wide_to_limbs / from_limbs, shamir_reconstruct_wide).
// "host": the restatement, the limb helpers and the reconstruction, no GPU.  No argument: the whole loop on the device -- secrets
// -> limb ciphertexts -> limb-wise sums of the dealers -> each party's aggregate share mod p -> the sum of the secrets.
// Built by tests/test_shamir_wide_host.py everywhere; the device half is run by tests/test_gpu_shamir_wide.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

// the order of the secp256k1 group
static const Wide SECP_N = {0xBFD25E8CD0364141ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, 0xFFFFFFFFFFFFFFFFULL};

static std::vector<Seed> make_seeds(size_t count) {
  std::vector<Seed> seeds(count);
  for (size_t d = 0; d < count; ++d) seeds[d].fill((uint8_t)(0x61 + d));
  return seeds;
}

// secrets far below p, so that their sum needs no reduction: dealer d's is d + 1 in word 3 and a pattern below
static std::vector<uint64_t> make_secrets(size_t D) {
  std::vector<uint64_t> s;
  for (size_t d = 0; d < D; ++d) {
    s.push_back(0x0123456789ABCDEFULL + d);
    s.push_back(~0ULL - 17 * d);
    s.push_back(0x8000000000000000ULL | d);
    s.push_back(d + 1);
  }
  return s;
}
// the sum of the secrets above as four words (D small: no carry out of word 3)
static std::vector<uint64_t> sum_of(const std::vector<uint64_t>& s) {
  std::vector<uint64_t> out(4, 0);
  for (size_t d = 0; d < s.size() / 4; ++d) {
    unsigned __int128 c = 0;
    for (int w = 0; w < 4; ++w) {
      c += (unsigned __int128)out[w] + s[d * 4 + w];
      out[w] = (uint64_t)c;
      c >>= 64;
    }
  }
  return out;
}

static int host_half() {
  const uint32_t n = 12, t = 4;
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const size_t D = 3;
  const std::vector<uint64_t> secrets = make_secrets(D);
  const std::vector<uint64_t> shares = shamir_shares_wide(params, secrets, t, SECP_N, make_seeds(D), {}, true);
  const std::vector<uint64_t> idx = {11, 0, 7, 3, 5};
  std::vector<uint64_t> picked;
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.insert(picked.end(), shares.begin() + (d * n + i) * 4, shares.begin() + (d * n + i + 1) * 4);
  if (shamir_reconstruct_wide(idx, picked, SECP_N) != secrets) {
    printf("reconstruction differs\n");
    return 1;
  }
  const uint32_t nl = shamir_wide_limbs(SECP_N, 52);
  if (nl != 5) return 1;
  if (shamir_wide_from_limbs(SECP_N, shamir_wide_to_limbs(shares, 52, nl), 52, nl) != shares) {
    printf("limb round trip differs\n");
    return 1;
  }
  bool refused = false;
  try {
    Wide even = SECP_N;
    even[0] -= 1;
    shamir_shares_wide(params, secrets, t, even, make_seeds(D), {}, true);
  } catch (const PvwError&) {
    refused = true;
  }
  if (!refused) return 1;
  printf("SHAMIR_WIDE_CPP_HOST_OK\n");
  return 0;
}

static int device_half() {
  const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
  const uint32_t n = 8, t = 3, limb_bits = 52;
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(4).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  Seed seed;
  seed.fill(0x3D);
  PvwCrs crs = PvwCrs::new_deterministic(params, seed);
  GlobalPublicKey global_pk(crs);
  std::vector<Party> parties;
  for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, seed));
  global_pk.generate_all_party_keys(parties, seed);
  const size_t D = 5;
  const uint32_t nl = shamir_wide_limbs(SECP_N, limb_bits);
  const std::vector<uint64_t> secrets = make_secrets(D);
  const std::vector<Seed> seeds = make_seeds(D * nl);
  std::vector<Seed> dealer_seeds;
  for (size_t d = 0; d < D; ++d) dealer_seeds.push_back(seeds[d * nl]);
  if (shamir_shares_wide(params, secrets, t, SECP_N, dealer_seeds) != shamir_shares_wide(params, secrets, t, SECP_N, dealer_seeds, {}, true)) {
    printf("device shares differ from the host's\n");
    return 1;
  }
  auto cts = deal_party_shares_wide(secrets, t, SECP_N, global_pk, seeds, limb_bits);
  // limb w of every dealer summed under encryption, every party's sum decrypted: sums [nl][n]
  std::vector<uint64_t> sums;
  for (uint32_t w = 0; w < nl; ++w) {
    std::vector<PvwCiphertext> plane;
    for (size_t d = 0; d < D; ++d) plane.push_back(cts[d * nl + w]);
    const CheckedShares r = decrypt_all_party_sums(plane, parties);
    sums.insert(sums.end(), r.values.begin(), r.values.end());
  }
  const std::vector<uint64_t> agg = shamir_wide_from_limbs(SECP_N, sums, limb_bits, nl);   // [n][4]
  const std::vector<uint64_t> idx = {6, 1, 4, 3};
  std::vector<uint64_t> picked;
  for (uint64_t i : idx) picked.insert(picked.end(), agg.begin() + i * 4, agg.begin() + (i + 1) * 4);
  if (shamir_reconstruct_wide(idx, picked, SECP_N) != sum_of(secrets)) {
    printf("the reconstructed sum differs\n");
    return 1;
  }
  printf("SHAMIR_WIDE_CPP_OK\n");
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

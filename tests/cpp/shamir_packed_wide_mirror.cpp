// Packed Shamir dealing over a 256-bit prime field through the C++ mirror (pvw_host::shamir_shares_packed_wide,
// deal_party_shares_packed_wide, shamir_reconstruct_packed_wide, shamir_reconstruct_packed_wide_corrected).
// "host": the restatement, the packed reconstruction, pack = 1 against shamir_shares_wide, the corrected way back on the host
// restatement, a refusal; no GPU.  No argument: the whole loop on the device -- pack secrets per dealer -> limb ciphertexts ->
// limb-wise sums of the dealers -> each party's aggregate share mod p -> the corrected sums of the secrets, with two parties'
// sums overwritten.
// Built by tests/test_shamir_packed_wide_host.py everywhere; the device half is run by tests/test_gpu_shamir_packed_wide.py.
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

// secrets far below p, so that the dealers' sums need no reduction: element e's is e + 1 in word 3 and a pattern below
static std::vector<uint64_t> make_secrets(size_t count) {
  std::vector<uint64_t> s;
  for (size_t e = 0; e < count; ++e) {
    s.push_back(0x0123456789ABCDEFULL + e);
    s.push_back(~0ULL - 17 * e);
    s.push_back(0x8000000000000000ULL | e);
    s.push_back(e + 1);
  }
  return s;
}
// sum over the dealers of secret j, [pack][4] (few dealers: no carry out of word 3)
static std::vector<uint64_t> sums_of(const std::vector<uint64_t>& s, size_t D, size_t K) {
  std::vector<uint64_t> out(K * 4, 0);
  for (size_t d = 0; d < D; ++d)
    for (size_t j = 0; j < K; ++j) {
      unsigned __int128 c = 0;
      for (int w = 0; w < 4; ++w) {
        c += (unsigned __int128)out[j * 4 + w] + s[(d * K + j) * 4 + w];
        out[j * 4 + w] = (uint64_t)c;
        c >>= 64;
      }
    }
  return out;
}

static int host_half() {
  const uint32_t n = 12, t = 4, K = 3;
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const size_t D = 3;
  const std::vector<uint64_t> secrets = make_secrets(D * K);
  const std::vector<uint64_t> shares = shamir_shares_packed_wide(params, secrets, K, t, SECP_N, make_seeds(D), {}, true);
  const std::vector<uint64_t> idx = {11, 0, 7, 3, 5, 9, 2};                     // t + K of them
  std::vector<uint64_t> picked;
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.insert(picked.end(), shares.begin() + (d * n + i) * 4, shares.begin() + (d * n + i + 1) * 4);
  if (shamir_reconstruct_packed_wide(idx, picked, SECP_N, K) != secrets) {
    printf("packed reconstruction differs\n");
    return 1;
  }
  const std::vector<uint64_t> singles = make_secrets(D);
  if (shamir_shares_packed_wide(params, singles, 1, t, SECP_N, make_seeds(D), {}, true) !=
      shamir_shares_wide(params, singles, t, SECP_N, make_seeds(D), {}, true)) {
    printf("pack 1 differs from the wide shares\n");
    return 1;
  }
  // the corrected way back on the host restatement: all n shares, two of row 1 bent
  std::vector<uint64_t> all(n), bent = shares;
  for (uint32_t i = 0; i < n; ++i) all[i] = i;
  bent[(1 * n + 4) * 4] ^= 1;
  bent[(1 * n + 10) * 4 + 3] ^= 1ULL << 40;
  const CorrectedPackedWideSecrets r = shamir_reconstruct_packed_wide_corrected(nullptr, SECP_N, K, t, all, bent, {}, false, true);
  if (r.secrets != secrets || r.report.nerr != std::vector<uint32_t>{0, 2, 0} || !r.report.wrong(1, 4) || !r.report.wrong(1, 10)) {
    printf("corrected packed reconstruction differs\n");
    return 1;
  }
  bool refused = false;
  try {
    shamir_shares_packed_wide(params, make_secrets(D * 9), 9, t, SECP_N, make_seeds(D), {}, true);   // degree + pack = n + 1
  } catch (const PvwError&) {
    refused = true;
  }
  if (!refused) return 1;
  printf("SHAMIR_PACKED_WIDE_CPP_HOST_OK\n");
  return 0;
}

static int device_half() {
  const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
  const uint32_t n = 12, t = 3, K = 3, limb_bits = 52;
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
  const std::vector<uint64_t> secrets = make_secrets(D * K);
  const std::vector<Seed> seeds = make_seeds(D * nl);
  std::vector<Seed> dealer_seeds;
  for (size_t d = 0; d < D; ++d) dealer_seeds.push_back(seeds[d * nl]);
  if (shamir_shares_packed_wide(params, secrets, K, t, SECP_N, dealer_seeds) !=
      shamir_shares_packed_wide(params, secrets, K, t, SECP_N, dealer_seeds, {}, true)) {
    printf("device shares differ from the host's\n");
    return 1;
  }
  auto cts = deal_party_shares_packed_wide(secrets, K, t, SECP_N, global_pk, seeds, limb_bits);
  // limb w of every dealer summed under encryption, every party's sum decrypted: sums [nl][n]
  std::vector<uint64_t> sums;
  for (uint32_t w = 0; w < nl; ++w) {
    std::vector<PvwCiphertext> plane;
    for (size_t d = 0; d < D; ++d) plane.push_back(cts[d * nl + w]);
    const CheckedShares r = decrypt_all_party_sums(plane, parties);
    sums.insert(sums.end(), r.values.begin(), r.values.end());
  }
  std::vector<uint64_t> agg = shamir_wide_from_limbs(SECP_N, sums, limb_bits, nl);   // [n][4]
  std::vector<uint64_t> all(n);
  for (uint32_t i = 0; i < n; ++i) all[i] = i;
  const std::vector<uint64_t> want = sums_of(secrets, D, K);
  CorrectedPackedWideSecrets r = shamir_reconstruct_packed_wide_corrected(params, SECP_N, K, t, all, agg);
  if (r.secrets != want || r.report.nerr[0] != 0) {
    printf("the reconstructed sums differ\n");
    return 1;
  }
  agg[2 * 4 + 1] ^= 0x10;
  for (int w = 0; w < 4; ++w) agg[7 * 4 + w] = 7;
  r = shamir_reconstruct_packed_wide_corrected(params, SECP_N, K, t, all, agg);
  if (r.secrets != want || r.report.nerr[0] != 2 || !r.report.wrong(0, 2) || !r.report.wrong(0, 7)) {
    printf("the corrected sums differ\n");
    return 1;
  }
  printf("SHAMIR_PACKED_WIDE_CPP_OK\n");
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

// Weighted sums of dealers' ciphertexts and the shares decrypted from them (pvw_host::combine_ciphertexts,
// decrypt_party_combination, decrypt_all_party_combinations, lincomb_fits, shamir_lagrange_weights).
// Built by tests/test_ct_lincomb_host.py everywhere; run on a machine with a GPU.
#include <cstdio>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

int main() {
  try {
    const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
    const uint32_t n = 8;
    const uint64_t p = (1ULL << 61) - 1;
    auto params = PvwParametersBuilder().set_parties(n).set_dimension(4).set_l(8).set_moduli(moduli)
                      .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
    Seed seed;
    seed.fill(0x3D);
    PvwCrs crs = PvwCrs::new_deterministic(params, seed);
    GlobalPublicKey global_pk(crs);
    std::vector<Party> parties;
    for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, seed));
    global_pk.generate_all_party_keys(parties, seed);
    std::vector<std::vector<uint64_t>> all(n);
    for (uint32_t d = 0; d < n; ++d)
      for (uint32_t j = 0; j < n; ++j) all[d].push_back(d * 1000 + j + 1);
    auto cts = encrypt_all_party_shares(all, global_pk, seed);
    const std::vector<bool> valid = {true, false, true, true, false, true, true, true};
    const std::vector<int64_t> weights = {3, 7, -1, 0, 5, 2, -4, 1};
    if (!lincomb_fits(params, weights, valid)) {
      printf("small weights do not fit\n");
      return 1;
    }
    const std::vector<int64_t> lam = shamir_lagrange_weights({0, 2, 5}, p);
    unsigned __int128 one_mod_p = 0;
    for (int64_t w : lam) one_mod_p += w < 0 ? p - (uint64_t)(-w) : (uint64_t)w;
    if (lam.size() != 3 || (uint64_t)(one_mod_p % p) != 1) {
      printf("the Lagrange weights at 0 do not sum to 1\n");
      return 1;
    }
    const pvw_plain_t plain{p, 0, nullptr};
    CheckedShares combos = decrypt_all_party_combinations(cts, weights, parties, valid, 0, &plain);
    PvwCiphertext comb = combine_ciphertexts(cts, weights, valid);
    for (uint32_t i = 0; i < n; ++i) {
      int64_t sum = 0;
      for (uint32_t d = 0; d < n; ++d) sum += valid[d] ? weights[d] * (int64_t)all[d][i] : 0;
      const uint64_t want = sum < 0 ? p - (uint64_t)(-sum) : (uint64_t)sum;
      CheckedShares one = decrypt_party_combination(cts, weights, parties[i].secret_key, i, valid, 0, &plain);
      if (combos.values[i] != want || one.values[0] != want || !combos.valid[i] || !one.valid[0] || one.noise[0] != combos.noise[i] ||
          combos.negative[i] != (sum < 0) || (sum >= 0 && decrypt_party_value(comb, parties[i].secret_key, i) != want)) {
        printf("party %u: %llu / %llu, expected %llu\n", i, (unsigned long long)combos.values[i], (unsigned long long)one.values[0],
               (unsigned long long)want);
        return 1;
      }
    }
    printf("CT_LINCOMB_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

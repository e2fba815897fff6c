// The sum of the valid dealers' ciphertexts and the aggregate shares decrypted from it (pvw_host::aggregate_ciphertexts,
// decrypt_party_sum, decrypt_all_party_sums): what examples/pvw_valid_dec.rs:150-209 reaches by decrypting every share.
// Built by tests/test_ct_sum_host.py everywhere; run on a machine with a GPU.
#include <cstdio>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

int main() {
  try {
    const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
    const uint32_t n = 8;
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
    CheckedShares sums = decrypt_all_party_sums(cts, parties, valid);
    PvwCiphertext agg = aggregate_ciphertexts(cts, valid);
    for (uint32_t i = 0; i < n; ++i) {
      uint64_t want = 0;
      for (uint32_t d = 0; d < n; ++d) want += valid[d] ? all[d][i] : 0;
      CheckedShares one = decrypt_party_sum(cts, parties[i].secret_key, i, valid);
      if (sums.values[i] != want || one.values[0] != want || !sums.valid[i] || !one.valid[0] || one.noise[0] != sums.noise[i] ||
          decrypt_party_value(agg, parties[i].secret_key, i) != want) {
        printf("party %u: %llu / %llu, expected %llu\n", i, (unsigned long long)sums.values[i], (unsigned long long)one.values[0],
               (unsigned long long)want);
        return 1;
      }
    }
    printf("CT_SUM_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

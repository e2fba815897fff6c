// Many weighted sums of the same dealers' ciphertexts (pvw_host::combine_ciphertexts_many, decrypt_all_party_combinations_many,
// shamir_lagrange_weights_at, shamir_packed_handover_weights).
// Built by tests/test_ct_lincomb_many_host.py everywhere; run on a machine with a GPU.
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
    // host only: the rows at the points 0 and -1 of the holders 0, 2, 5; the row at 0 is shamir_lagrange_weights
    const std::vector<std::vector<int64_t>> lam = shamir_packed_handover_weights({0, 2, 5}, p, 2);
    if (lam.size() != 2 || lam[0] != shamir_lagrange_weights({0, 2, 5}, p) || shamir_lagrange_weights_at({0, 2, 5}, {2}, p)[0] != std::vector<int64_t>{0, 1, 0}) {
      printf("the weights at the points 0 / -1 / an index are wrong\n");
      return 1;
    }
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
    const std::vector<std::vector<int64_t>> rows = {{3, 7, -1, 0, 5, 2, -4, 1}, {0, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1, 1, 1}};
    const pvw_plain_t plain{p, 0, nullptr};
    CheckedShares many = decrypt_all_party_combinations_many(cts, rows, parties, valid, 0, &plain);
    std::vector<PvwCiphertext> combs = combine_ciphertexts_many(cts, rows, valid);
    const size_t R = rows.size();
    for (size_t r = 0; r < R; ++r) {
      const bool empty = r == 1;
      CheckedShares one;
      PvwCiphertext comb;
      if (!empty) {
        one = decrypt_all_party_combinations(cts, rows[r], parties, valid, 0, &plain);
        comb = combine_ciphertexts(cts, rows[r], valid);
        if (comb.c1 != combs[r].c1 || comb.c2 != combs[r].c2) {
          printf("row %zu: the combined ciphertext differs from combine_ciphertexts\n", r);
          return 1;
        }
      }
      for (uint32_t i = 0; i < n; ++i) {
        int64_t sum = 0;
        for (uint32_t d = 0; d < n; ++d) sum += valid[d] ? rows[r][d] * (int64_t)all[d][i] : 0;
        const uint64_t want = sum < 0 ? p - (uint64_t)(-sum) : (uint64_t)sum;
        if (many.values[i * R + r] != want || !many.valid[i * R + r] ||
            (!empty && (one.values[i] != want || one.noise[i] != many.noise[i * R + r]))) {
          printf("party %u row %zu: %llu, expected %llu\n", i, r, (unsigned long long)many.values[i * R + r], (unsigned long long)want);
          return 1;
        }
      }
    }
    printf("CT_LINCOMB_MANY_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

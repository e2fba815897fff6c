// Every party decrypts its share from every dealer in one call (pvw_host::decrypt_all_party_shares), as
// examples/pvw.rs:138-170 does party by party, and over a subset of dealers (decrypt_many, examples/pvw_valid_dec.rs:201-209).
// Built by tests/test_decrypt_all_host.py everywhere; run there on the GPU box.
#include <cstdio>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

int main() {
  try {
    const std::vector<uint64_t> moduli = {0xffffee001ULL, 0xffffc4001ULL, 0x1ffffe0001ULL};
    const uint32_t n = 24;
    auto [bound1, bound2] = PvwParameters::suggest_error_bounds(n, 4, 16, moduli, 0.5f);
    auto params = PvwParametersBuilder().set_parties(n).set_dimension(4).set_l(16).set_moduli(moduli)
                      .set_secret_variance(0.5f).set_error_bounds_u32(bound1, bound2).build_arc();
    Seed seed;
    seed.fill(0x5C);
    PvwCrs crs = PvwCrs::new_deterministic(params, seed);
    GlobalPublicKey global_pk(crs);
    std::vector<Party> parties;
    for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, seed));
    global_pk.generate_all_party_keys(parties, seed);
    std::vector<std::vector<uint64_t>> all(n);
    for (uint32_t d = 0; d < n; ++d)
      for (uint32_t j = 0; j < n; ++j) all[d].push_back(d * 1000 + j + 1);
    auto cts = encrypt_all_party_shares(all, global_pk, seed);
    // results[recipient][dealer]: equal to the per-party path, word for word
    auto res = decrypt_all_party_shares(cts, parties);
    uint32_t correct = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (res[i] != decrypt_party_shares(cts, parties[i].secret_key, i)) { printf("party %u differs from decrypt_party_shares\n", i); return 1; }
      for (uint32_t d = 0; d < n; ++d) correct += res[i][d] == all[d][i];
    }
    if (correct < n * n * 95 / 100) { printf("only %u of %u shares recovered\n", correct, n * n); return 1; }
    // a subset of dealers for the parties [3, 20)
    std::vector<PvwCiphertext> valid = {cts[7], cts[2], cts[19]};
    std::vector<const SecretKey*> keys;
    for (uint32_t i = 3; i < 20; ++i) keys.push_back(&parties[i].secret_key);
    auto sub = decrypt_many(valid, keys, 3);
    for (uint32_t i = 3; i < 20; ++i)
      if (sub[i - 3] != std::vector<uint64_t>{res[i][7], res[i][2], res[i][19]}) { printf("subset mismatch at party %u\n", i); return 1; }
    printf("DECRYPT_ALL_CPP_OK %u/%u\n", correct, n * n);
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

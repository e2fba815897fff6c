// Corrected reconstruction through the C++ mirror (pvw_host::shamir_reconstruct_corrected).
// "host": the plain restatement, no GPU -- a clean sharing, E wrong shares in one row (two of them among the first t + 1
// columns), both layouts, E + 1 wrong shares, a refusal.  No argument: the same cases on the device, each compared with the host.
// Built by tests/test_shamir_correct_host.py everywhere; the device half is run by tests/test_gpu_shamir_correct.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

static const uint64_t P61 = (1ULL << 61) - 1;

static bool same(const CorrectedSecrets& a, const CorrectedSecrets& b) {
  return a.secrets == b.secrets && a.nerr == b.nerr && a.col_err == b.col_err && a.err_mask == b.err_mask && a.words == b.words;
}

static int run_cases(const std::shared_ptr<PvwParameters>& params, bool host) {
  const uint32_t n = 12, t = 4, E = 3;                  // r = 7
  const size_t D = 3;
  const std::vector<uint64_t> secrets = {5, ~0ULL, P61 + 3};
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x51 + d));
  const std::vector<uint64_t> shares = shamir_shares(params, secrets, t, P61, seeds, {}, true);
  std::vector<uint64_t> idx, picked;
  for (uint32_t i = 0; i < n; ++i) idx.push_back((i * 7 + 2) % n);   // 7 is a unit mod 12: a permutation
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.push_back(shares[d * n + i]);
  auto both = [&](const std::vector<uint64_t>& sh, CorrectedSecrets& r) {
    r = shamir_reconstruct_corrected(params, idx, sh, t, P61, host);
    return host || same(r, shamir_reconstruct_corrected(params, idx, sh, t, P61, true));
  };
  CorrectedSecrets r;
  if (!both(picked, r)) return 1;
  for (size_t d = 0; d < D; ++d)
    if (r.secrets[d] != secrets[d] % P61 || r.nerr[d] != 0 || r.err_mask[d] != 0) return 2;
  for (uint32_t v : r.col_err)
    if (v != 0) return 3;
  // E wrong shares in row 1, two of them among the first t + 1 columns; one in row 2
  std::vector<uint64_t> bent = picked;
  const size_t wrong[3] = {0, 3, 9};
  for (size_t c : wrong) bent[1 * n + c] += 1 + c;
  bent[2 * n + 3] ^= 2;
  if (!both(bent, r)) return 4;
  for (size_t d = 0; d < D; ++d)
    if (r.secrets[d] != secrets[d] % P61) return 5;
  if (r.nerr[0] != 0 || r.nerr[1] != E || r.nerr[2] != 1) return 6;
  for (size_t c = 0; c < n; ++c) {
    const bool w1 = c == 0 || c == 3 || c == 9;
    if (r.wrong(1, c) != w1 || r.wrong(2, c) != (c == 3) || r.wrong(0, c)) return 7;
    if (r.col_err[c] != (uint32_t)w1 + (c == 3)) return 8;
  }
  // party-major: the transposed matrix gives the same report
  std::vector<uint64_t> tr(bent.size());
  for (size_t d = 0; d < D; ++d)
    for (size_t i = 0; i < n; ++i) tr[i * D + d] = bent[d * n + i];
  if (!same(shamir_reconstruct_corrected(params, idx, tr, t, P61, host, true), r)) return 9;
  // E + 1 wrong shares: no polynomial within E columns (a false decode at this p has probability about 2^-61 n^E)
  bent[1 * n + 5] += 77;
  if (!both(bent, r)) return 10;
  if (r.nerr[1] != PVW_SHAMIR_UNDECODABLE || r.secrets[1] != 0 || r.err_mask[1] != 0) return 11;
  if (r.secrets[0] != secrets[0] % P61 || r.secrets[2] != secrets[2] % P61 || r.col_err[3] != 1 || r.col_err[0] != 0) return 12;
  bool refused = false;
  try {
    std::vector<uint64_t> dup = idx;
    dup[3] = dup[0];
    shamir_reconstruct_corrected(params, dup, picked, t, P61, host);
  } catch (const PvwError&) {
    refused = true;
  }
  return refused ? 0 : 13;
}

int main(int argc, char** argv) {
  try {
    const bool host = argc > 1 && !strcmp(argv[1], "host");
    const std::vector<uint64_t> moduli = host ? std::vector<uint64_t>{0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL}
                                              : std::vector<uint64_t>{0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
    auto params = PvwParametersBuilder().set_parties(12).set_dimension(host ? 2 : 4).set_l(8).set_moduli(moduli)
                      .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
    const int rc = run_cases(params, host);
    if (rc) {
      printf("%s case %d failed\n", host ? "host" : "device", rc);
      return 1;
    }
    printf(host ? "CORRECT_CPP_HOST_OK\n" : "CORRECT_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

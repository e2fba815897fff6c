// Share repair through the C++ mirror (pvw_host::shamir_evaluate_corrected).
// "host": the plain restatement, no GPU -- a clean sharing evaluated at every party, E wrong shares in one row repaired, a party
// that was never an input, both layouts, E + 1 wrong shares (a zero row), a refusal.  No argument: the same cases on the device,
// each compared with the host.
// Built by tests/test_shamir_evaluate_host.py everywhere; the device half is run by tests/test_gpu_shamir_evaluate.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

static const uint64_t P61 = (1ULL << 61) - 1;

static bool same(const EvaluatedShares& a, const EvaluatedShares& b) {
  return a.values == b.values && a.decode.secrets == b.decode.secrets && a.decode.nerr == b.decode.nerr &&
         a.decode.col_err == b.decode.col_err && a.decode.err_mask == b.decode.err_mask && a.decode.words == b.decode.words;
}

static int run_cases(const std::shared_ptr<PvwParameters>& params, bool host) {
  const uint32_t n = 12, used = 11, t = 4, E = 3;       // party 11 is no input: count = 11, r = 6
  const size_t D = 3;
  const std::vector<uint64_t> secrets = {5, ~0ULL, P61 + 3};
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x61 + d));
  const std::vector<uint64_t> shares = shamir_shares(params, secrets, t, P61, seeds, {}, true);   // [D][n]
  std::vector<uint64_t> idx, picked, targets;
  for (uint32_t i = 0; i < used; ++i) idx.push_back((i * 7 + 2) % used);   // 7 is a unit mod 11: a permutation of 0..10
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.push_back(shares[d * n + i]);
  for (uint32_t i = 0; i < n; ++i) targets.push_back(i);                   // every party, the one without an input included
  targets.push_back(3);                                                    // and one twice
  const size_t T = targets.size();
  auto both = [&](const std::vector<uint64_t>& sh, EvaluatedShares& r) {
    r = shamir_evaluate_corrected(params, idx, sh, t, P61, targets, host);
    return host || same(r, shamir_evaluate_corrected(params, idx, sh, t, P61, targets, true));
  };
  auto dealt = [&](const EvaluatedShares& r, size_t d) {
    for (size_t j = 0; j < T; ++j)
      if (r.values[d * T + j] != shares[d * n + targets[j]]) return false;
    return true;
  };
  EvaluatedShares r;
  if (!both(picked, r)) return 1;
  for (size_t d = 0; d < D; ++d)
    if (!dealt(r, d) || r.decode.secrets[d] != secrets[d] % P61 || r.decode.nerr[d] != 0) return 2;
  // E wrong shares in row 1, two of them among the first t + 1 columns; one in row 2: every value is still the dealt share
  std::vector<uint64_t> bent = picked;
  const size_t wrong[3] = {0, 3, 9};
  for (size_t c : wrong) bent[1 * used + c] += 1 + c;
  bent[2 * used + 3] ^= 2;
  if (!both(bent, r)) return 3;
  for (size_t d = 0; d < D; ++d)
    if (!dealt(r, d) || r.decode.secrets[d] != secrets[d] % P61) return 4;
  if (r.decode.nerr[0] != 0 || r.decode.nerr[1] != E || r.decode.nerr[2] != 1) return 5;
  for (size_t c = 0; c < used; ++c)
    if (r.decode.wrong(1, c) != (c == 0 || c == 3 || c == 9) || r.decode.wrong(2, c) != (c == 3)) return 6;
  // the four reports are those of the corrected call
  {
    const CorrectedSecrets c = shamir_reconstruct_corrected(params, idx, bent, t, P61, host);
    if (c.secrets != r.decode.secrets || c.nerr != r.decode.nerr || c.col_err != r.decode.col_err || c.err_mask != r.decode.err_mask) return 7;
  }
  // party-major: the transposed matrix gives the same report
  std::vector<uint64_t> tr(bent.size());
  for (size_t d = 0; d < D; ++d)
    for (size_t i = 0; i < used; ++i) tr[i * D + d] = bent[d * used + i];
  if (!same(shamir_evaluate_corrected(params, idx, tr, t, P61, targets, host, true), r)) return 8;
  // E + 1 wrong shares: no polynomial within E columns (a false decode at this p has probability about 2^-61 n^E): a zero row
  bent[1 * used + 5] += 77;
  if (!both(bent, r)) return 9;
  if (r.decode.nerr[1] != PVW_SHAMIR_UNDECODABLE || r.decode.secrets[1] != 0) return 10;
  for (size_t j = 0; j < T; ++j)
    if (r.values[1 * T + j] != 0) return 11;
  if (!dealt(r, 0) || !dealt(r, 2)) return 12;
  bool refused = false;
  try {
    std::vector<uint64_t> far = targets;
    far[2] = P61 - 1;                                   // its point would be p
    shamir_evaluate_corrected(params, idx, picked, t, P61, far, host);
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
    printf(host ? "EVALUATE_CPP_HOST_OK\n" : "EVALUATE_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

// Share repair over a 256-bit prime field through the C++ mirror (pvw_host::shamir_evaluate_wide_corrected).
// "host": the plain C++ restatement on a consistent sharing with erased columns full of junk and wrong shares beside them: the
// values at every party's index are the dealt shares, the report is that of shamir_reconstruct_wide_corrected, an undecodable row
// is 0, no GPU.
// No argument: the same matrices through the device form, compared with the restatement word for word.
// Built by tests/test_shamir_wide_evaluate_host.py everywhere; the device half is run by tests/test_gpu_shamir_wide_evaluate.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

// the order of the secp256k1 group
static const Wide SECP_N = {0xBFD25E8CD0364141ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, 0xFFFFFFFFFFFFFFFFULL};

static std::shared_ptr<PvwParameters> make_params(uint32_t n) {
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  return PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(moduli)
      .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
}

static bool same(const CorrectedWideSecrets& a, const CorrectedWideSecrets& b) {
  return a.secrets == b.secrets && a.nerr == b.nerr && a.col_err == b.col_err && a.err_mask == b.err_mask && a.words == b.words;
}

static int check_repair(const std::shared_ptr<PvwParameters>& params, bool host) {
  const uint32_t n = 12, t = 2;
  const size_t D = 4;
  const std::vector<uint64_t> idx = {9, 0, 7, 3, 5, 11, 2};       // r = 4
  const size_t count = idx.size();
  std::vector<uint64_t> secrets;
  for (size_t d = 0; d < D; ++d) {
    secrets.push_back(0x0123456789ABCDEFULL + d);
    secrets.push_back(~0ULL - 17 * d);
    secrets.push_back(0x8000000000000000ULL | d);
    secrets.push_back(d + 1);
  }
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x71 + d));
  const std::vector<uint64_t> all = shamir_shares_wide(params, secrets, t, SECP_N, seeds, {}, true);   // [D][n][4]
  std::vector<uint64_t> sh;
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) sh.insert(sh.end(), all.begin() + (d * n + i) * 4, all.begin() + (d * n + i + 1) * 4);
  std::vector<uint64_t> targets(n);
  for (uint32_t i = 0; i < n; ++i) targets[i] = i;
  // secret 0: four erasures; secret 1: two erasures and one error; secret 2: two errors, no mask bit; secret 3: five erasures (> r)
  std::vector<uint64_t> erased(D, 0);
  auto erase = [&](size_t s, size_t k) {
    erased[s] |= 1ULL << k;
    for (int w = 0; w < 4; ++w) sh[(s * count + k) * 4 + w] = ~0ULL;
  };
  for (size_t k : {0, 2, 3, 6}) erase(0, k);
  for (size_t k : {1, 5}) erase(1, k);
  sh[(1 * count + 0) * 4 + 3] ^= 4;
  sh[(2 * count + 4) * 4 + 1] ^= 1;
  sh[(2 * count + 6) * 4 + 0] += 5;
  for (size_t k : {0, 1, 2, 3, 4}) erase(3, k);
  const EvaluatedWideShares e = shamir_evaluate_wide_corrected(params, idx, sh, t, SECP_N, targets, erased, false, host);
  if (!same(e.report, shamir_reconstruct_wide_corrected(params, idx, sh, t, SECP_N, erased, false, host))) {
    printf("the report is not the decode-only call's\n");
    return 1;
  }
  if (e.report.nerr != std::vector<uint32_t>{0, 1, 2, PVW_SHAMIR_UNDECODABLE}) {
    printf("the report is not what was planted\n");
    return 1;
  }
  for (size_t d = 0; d < D; ++d)
    for (size_t j = 0; j < n * 4; ++j)
      if (e.values[d * n * 4 + j] != (d == 3 ? 0 : all[d * n * 4 + j])) {
        printf("secret %zu: the values are not the dealt shares\n", d);
        return 1;
      }
  // party-major, and a duplicate target; without a mask secret 0 is beyond E and its row of values is 0
  std::vector<uint64_t> tr(sh.size());
  for (size_t d = 0; d < D; ++d)
    for (size_t k = 0; k < count; ++k) memcpy(&tr[(k * D + d) * 4], &sh[(d * count + k) * 4], 32);
  const EvaluatedWideShares p2 = shamir_evaluate_wide_corrected(params, idx, tr, t, SECP_N, targets, erased, true, host);
  if (p2.values != e.values || !same(p2.report, e.report)) {
    printf("the party-major result differs\n");
    return 1;
  }
  const EvaluatedWideShares m = shamir_evaluate_wide_corrected(params, idx, sh, t, SECP_N, {4, 4, 100}, {}, false, host);
  if (m.report.nerr[0] != PVW_SHAMIR_UNDECODABLE || m.values[0] || m.values[11] || m.report.nerr[2] != 2 ||
      memcmp(&m.values[2 * 3 * 4], &m.values[(2 * 3 + 1) * 4], 32) || memcmp(&m.values[2 * 3 * 4], &all[(2 * n + 4) * 4], 32)) {
    printf("the maskless result is wrong\n");
    return 1;
  }
  if (!host) {
    const EvaluatedWideShares h = shamir_evaluate_wide_corrected(params, idx, sh, t, SECP_N, targets, erased, false, true);
    const EvaluatedWideShares hm = shamir_evaluate_wide_corrected(params, idx, sh, t, SECP_N, {4, 4, 100}, {}, false, true);
    if (h.values != e.values || !same(h.report, e.report) || hm.values != m.values || !same(hm.report, m.report)) {
      printf("the device result differs from the host's\n");
      return 1;
    }
  }
  bool refused = false;
  try {
    shamir_evaluate_wide_corrected(params, idx, sh, t, SECP_N, {}, erased, false, host);   // no targets
  } catch (const PvwError&) {
    refused = true;
  }
  return refused ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    const bool host = argc > 1 && !strcmp(argv[1], "host");
    auto params = make_params(12);
    if (check_repair(params, host)) return 1;
    printf(host ? "SHAMIR_WIDE_EVALUATE_CPP_HOST_OK\n" : "SHAMIR_WIDE_EVALUATE_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

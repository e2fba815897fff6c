// Wide share repair at field points through the C++ mirror (pvw_host::shamir_evaluate_wide_corrected_at,
// pvw_host::shamir_packed_wide_secrets).
// "host": the plain C++ restatement on packed sharings dealt by shamir_shares_packed_wide with erased columns full of junk and
// wrong shares beside them: the packed call returns the dealt secrets, equals the older route through corrected shares
// (shamir_reconstruct_packed_wide_corrected) and the evaluation at the points 0, p - 1, p - 2; an undecodable row is 0; no GPU.
// No argument: the same matrices through the device forms, compared with the restatement word for word.
// Built by tests/test_shamir_wide_points_host.py everywhere; the device half is run by tests/test_gpu_shamir_wide_points.py.
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
  return a.nerr == b.nerr && a.col_err == b.col_err && a.err_mask == b.err_mask && a.words == b.words;
}

static int check_packed(const std::shared_ptr<PvwParameters>& params, bool host) {
  const uint32_t n = 12, t = 2, K = 3;
  const size_t D = 4;
  const std::vector<uint64_t> idx = {9, 0, 7, 3, 5, 11, 2, 4, 10};   // r = 9 - 2 - 3 = 4
  const size_t count = idx.size();
  std::vector<uint64_t> secrets;                                      // [D][K][4], below p
  for (size_t d = 0; d < D; ++d)
    for (uint32_t m = 0; m < K; ++m) {
      secrets.push_back(0x0123456789ABCDEFULL + d + 7 * m);
      secrets.push_back(~0ULL - 17 * d - m);
      secrets.push_back(0x8000000000000000ULL | (d << 8) | m);
      secrets.push_back(d + 1 + m);
    }
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x51 + d));
  const std::vector<uint64_t> all = shamir_shares_packed_wide(params, secrets, K, t, SECP_N, seeds, {}, true);   // [D][n][4]
  std::vector<uint64_t> sh;
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) sh.insert(sh.end(), all.begin() + (d * n + i) * 4, all.begin() + (d * n + i + 1) * 4);
  // row 0: four erasures; row 1: two erasures and one error; row 2: two errors, no mask bit; row 3: five erasures (> r)
  std::vector<uint64_t> erased(D, 0);
  auto erase = [&](size_t s, size_t k) {
    erased[s] |= 1ULL << k;
    for (int w = 0; w < 4; ++w) sh[(s * count + k) * 4 + w] = ~0ULL;
  };
  for (size_t k : {0, 2, 3, 6}) erase(0, k);
  for (size_t k : {1, 5}) erase(1, k);
  sh[(1 * count + 0) * 4 + 3] ^= 4;
  sh[(2 * count + 4) * 4 + 1] ^= 1;
  sh[(2 * count + 8) * 4 + 0] += 5;
  for (size_t k : {0, 1, 2, 3, 4}) erase(3, k);
  const CorrectedPackedWideSecrets got = shamir_packed_wide_secrets(params, SECP_N, K, t, idx, sh, erased, false, host);
  if (got.report.nerr != std::vector<uint32_t>{0, 1, 2, PVW_SHAMIR_UNDECODABLE}) {
    printf("the report is not what was planted\n");
    return 1;
  }
  for (size_t d = 0; d < D; ++d)
    for (size_t j = 0; j < K * 4; ++j)
      if (got.secrets[d * K * 4 + j] != (d == 3 ? 0 : secrets[d * K * 4 + j])) {
        printf("row %zu: the secrets are not the dealt ones\n", d);
        return 1;
      }
  const CorrectedPackedWideSecrets old = shamir_reconstruct_packed_wide_corrected(params, SECP_N, K, t, idx, sh, erased, false, host);
  if (old.secrets != got.secrets || !same(old.report, got.report)) {
    printf("the route through corrected shares differs\n");
    return 1;
  }
  // the same polynomials at the points 0, p - 1, p - 2 and on a column; the point 0 is the decode's secret
  std::vector<uint64_t> points = {0, 0, 0, 0};
  for (uint64_t m = 1; m < K; ++m) points.insert(points.end(), {SECP_N[0] - m, SECP_N[1], SECP_N[2], SECP_N[3]});
  points.insert(points.end(), {idx[4] + 1, 0, 0, 0});
  const EvaluatedWideShares ev = shamir_evaluate_wide_corrected_at(params, idx, sh, t + K - 1, SECP_N, points, erased, false, host);
  if (!same(ev.report, got.report)) {
    printf("the evaluation's report differs\n");
    return 1;
  }
  for (size_t d = 0; d < D; ++d) {
    if (memcmp(&ev.values[d * (K + 1) * 4], &got.secrets[d * K * 4], K * 32) || memcmp(&ev.values[d * (K + 1) * 4], &ev.report.secrets[d * 4], 32)) {
      printf("row %zu: the values at 0, -1, .. are not the secrets\n", d);
      return 1;
    }
    if (d != 3 && memcmp(&ev.values[(d * (K + 1) + K) * 4], &all[(d * n + idx[4]) * 4], 32)) {   // wrong in row 2: the dealt share
      printf("row %zu: the value on a column is not the dealt share\n", d);
      return 1;
    }
  }
  // party-major, and without a mask: row 0 is beyond the bound then
  std::vector<uint64_t> tr(sh.size());
  for (size_t d = 0; d < D; ++d)
    for (size_t k = 0; k < count; ++k) memcpy(&tr[(k * D + d) * 4], &sh[(d * count + k) * 4], 32);
  const CorrectedPackedWideSecrets p2 = shamir_packed_wide_secrets(params, SECP_N, K, t, idx, tr, erased, true, host);
  if (p2.secrets != got.secrets || !same(p2.report, got.report)) {
    printf("the party-major result differs\n");
    return 1;
  }
  const CorrectedPackedWideSecrets m = shamir_packed_wide_secrets(params, SECP_N, K, t, idx, sh, {}, false, host);
  if (m.report.nerr[0] != PVW_SHAMIR_UNDECODABLE || m.secrets[0] || m.report.nerr[2] != 2 ||
      memcmp(&m.secrets[2 * K * 4], &secrets[2 * K * 4], K * 32)) {
    printf("the maskless result is wrong\n");
    return 1;
  }
  if (!host) {
    const CorrectedPackedWideSecrets h = shamir_packed_wide_secrets(params, SECP_N, K, t, idx, sh, erased, false, true);
    const EvaluatedWideShares he = shamir_evaluate_wide_corrected_at(params, idx, sh, t + K - 1, SECP_N, points, erased, false, true);
    if (h.secrets != got.secrets || !same(h.report, got.report) || he.values != ev.values || !same(he.report, ev.report) ||
        he.report.secrets != ev.report.secrets) {
      printf("the device result differs from the host's\n");
      return 1;
    }
  }
  int refused = 0;
  try {
    shamir_packed_wide_secrets(params, SECP_N, 0, t, idx, sh, erased, false, host);             // pack = 0
  } catch (const PvwError&) {
    ++refused;
  }
  try {
    points[4] = SECP_N[0];                                                                       // a point equal to p
    shamir_evaluate_wide_corrected_at(params, idx, sh, t + K - 1, SECP_N, points, erased, false, host);
  } catch (const PvwError&) {
    ++refused;
  }
  return refused == 2 ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    const bool host = argc > 1 && !strcmp(argv[1], "host");
    auto params = make_params(12);
    if (check_packed(params, host)) return 1;
    printf(host ? "SHAMIR_WIDE_POINTS_CPP_HOST_OK\n" : "SHAMIR_WIDE_POINTS_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

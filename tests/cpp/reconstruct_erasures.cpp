// Reconstruction with erasures through the C++ mirror (the pvw_host::shamir_reconstruct_corrected / shamir_evaluate_corrected
// overloads that take `erased`, and pvw_host::shamir_erasure_mask).
// "host": the plain restatement, no GPU -- r erased shares filled with junk and no error, erasures plus errors at the bound and one
// error beyond it, an err_mask fed back as erased, an empty mask (the corrected call), the mask of a report, both layouts, a refusal.
// No argument: the same cases on the device, each compared with the host.
// Built by tests/test_shamir_erasures_host.py everywhere; the device half is run by tests/test_gpu_shamir_erasures.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

static const uint64_t P61 = (1ULL << 61) - 1;

static bool same(const CorrectedSecrets& a, const CorrectedSecrets& b) {
  return a.secrets == b.secrets && a.nerr == b.nerr && a.col_err == b.col_err && a.err_mask == b.err_mask && a.words == b.words;
}
static bool same(const EvaluatedShares& a, const EvaluatedShares& b) { return a.values == b.values && same(a.decode, b.decode); }

static int run_cases(const std::shared_ptr<PvwParameters>& params, bool host) {
  const uint32_t n = 12, used = 11, t = 4;              // party 11 is no input: count = 11, r = 6
  const size_t D = 3;
  const std::vector<uint64_t> secrets = {5, ~0ULL, P61 + 3};
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x71 + d));
  const std::vector<uint64_t> shares = shamir_shares(params, secrets, t, P61, seeds, {}, true);   // [D][n]
  std::vector<uint64_t> idx, picked, targets;
  for (uint32_t i = 0; i < used; ++i) idx.push_back((i * 7 + 2) % used);
  for (size_t d = 0; d < D; ++d)
    for (uint64_t i : idx) picked.push_back(shares[d * n + i]);
  for (uint32_t i = 0; i < n; ++i) targets.push_back(i);
  targets.push_back(3);
  const size_t T = targets.size();
  auto both = [&](const std::vector<uint64_t>& sh, const std::vector<uint64_t>& er, EvaluatedShares& r) {
    r = shamir_evaluate_corrected(params, idx, sh, t, P61, targets, er, host);
    if (!same(shamir_reconstruct_corrected(params, idx, sh, t, P61, er, host), r.decode)) return false;
    return host || same(r, shamir_evaluate_corrected(params, idx, sh, t, P61, targets, er, true));
  };
  auto dealt = [&](const EvaluatedShares& r, size_t d) {
    for (size_t j = 0; j < T; ++j)
      if (r.values[d * T + j] != shares[d * n + targets[j]]) return false;
    return true;
  };
  // row 0: six erased shares (r of them) and no error; row 1: two erased, two wrong (2 + 2 * 2 = r); row 2: nothing erased, one wrong
  std::vector<uint64_t> bent = picked, er(D, 0);
  for (size_t c : {0, 2, 3, 5, 8, 10}) bent[0 * used + c] = ~0ULL - c, er[0] |= 1ULL << c;
  for (size_t c : {1, 9}) bent[1 * used + c] = 0x1234567 + c, er[1] |= 1ULL << c;
  for (size_t c : {0, 4}) bent[1 * used + c] += 1 + c;
  bent[2 * used + 3] ^= 2;
  er[2] |= ~0ULL << used;                               // padding bits are ignored
  EvaluatedShares r;
  if (!both(bent, er, r)) return 1;
  for (size_t d = 0; d < D; ++d)
    if (!dealt(r, d) || r.decode.secrets[d] != secrets[d] % P61) return 2;
  if (r.decode.nerr[0] != 0 || r.decode.nerr[1] != 2 || r.decode.nerr[2] != 1) return 3;
  for (size_t c = 0; c < used; ++c)
    if (r.decode.wrong(0, c) || r.decode.wrong(1, c) != (c == 0 || c == 4) || r.decode.wrong(2, c) != (c == 3)) return 4;
  // without the mask row 0 has six bad shares and row 1 four: beyond E = 3
  {
    const CorrectedSecrets c = shamir_reconstruct_corrected(params, idx, bent, t, P61, host);
    if (c.nerr[0] != PVW_SHAMIR_UNDECODABLE || c.nerr[1] != PVW_SHAMIR_UNDECODABLE || c.nerr[2] != 1) return 5;
    // an empty mask is that call
    if (!same(shamir_reconstruct_corrected(params, idx, bent, t, P61, std::vector<uint64_t>(), host), c)) return 6;
  }
  // the err_mask fed back as erased (with the first mask): no error is left, the same secrets
  {
    std::vector<uint64_t> again = er;
    for (size_t d = 0; d < D; ++d) again[d] |= r.decode.err_mask[d];
    EvaluatedShares r2;
    if (!both(bent, again, r2)) return 7;
    if (r2.decode.secrets != r.decode.secrets || r2.values != r.values) return 8;
    for (size_t d = 0; d < D; ++d)
      if (r2.decode.nerr[d] != 0) return 9;
  }
  // party-major: the transposed matrix gives the same report
  std::vector<uint64_t> tr(bent.size());
  for (size_t d = 0; d < D; ++d)
    for (size_t i = 0; i < used; ++i) tr[i * D + d] = bent[d * used + i];
  if (!same(shamir_evaluate_corrected(params, idx, tr, t, P61, targets, er, host, true), r)) return 10;
  // one more wrong share in row 1: 2 + 2 * 3 > r, a zero row; seven erased in row 0: more than r
  bent[1 * used + 6] += 77;
  er[0] |= 1ULL << 1;
  if (!both(bent, er, r)) return 11;
  for (size_t d = 0; d < 2; ++d) {
    if (r.decode.nerr[d] != PVW_SHAMIR_UNDECODABLE || r.decode.secrets[d] != 0 || r.decode.err_mask[d] != 0) return 12;
    for (size_t j = 0; j < T; ++j)
      if (r.values[d * T + j] != 0) return 13;
  }
  if (!dealt(r, 2)) return 14;
  // the mask of a report: status bit 1 or noise above the bound, in both layouts
  {
    const std::vector<uint32_t> status = {0, 1, 2, 0, 0, 3};      // [2][3]
    const std::vector<uint64_t> noise = {9, 0, 0, 10, 11, 0};
    const std::vector<uint64_t> m = shamir_erasure_mask(status, noise, 3, 1, 10);
    if (m != std::vector<uint64_t>{0b010, 0b110}) return 15;
    const std::vector<uint64_t> mt = shamir_erasure_mask(status, noise, 2, 1, 10, true);   // the same cells as [count = 2][3 secrets]
    if (mt != std::vector<uint64_t>{0b00, 0b11, 0b10}) return 16;
  }
  bool refused = false;
  try {
    shamir_reconstruct_corrected(params, idx, picked, t, P61, std::vector<uint64_t>(D + 1, 0), host);   // a mask of another shape
  } catch (const PvwError&) {
    refused = true;
  }
  return refused ? 0 : 17;
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
    printf(host ? "ERASURES_CPP_HOST_OK\n" : "ERASURES_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

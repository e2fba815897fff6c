// Corrected reconstruction over a 256-bit prime field through the C++ mirror (pvw_host::shamir_reconstruct_wide_corrected;
// DESIGN 8.20).
// "host": the plain C++ restatement on a consistent sharing, with wrong shares inside and outside the first t + 1 columns and
// with one more than can be corrected, no GPU.
// No argument: the same matrices through the device form, compared with the restatement word for word.
// Built by tests/test_shamir_wide_corrected_host.py everywhere; the device half is run by tests/test_gpu_shamir_wide_corrected.py.
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

struct Case {
  std::vector<uint64_t> idx, shares, secrets;   // shares [D][count][4]
  size_t D, count;
  uint32_t t;
};

// D sharings of degree t over n parties (the host restatement of the dealing end), the columns of `idx` picked out
static Case make_case(const std::shared_ptr<PvwParameters>& params) {
  Case c;
  c.D = 5, c.t = 2;
  c.idx = {9, 0, 7, 3, 5, 11, 2};                // r = 4, E = 2
  c.count = c.idx.size();
  for (size_t d = 0; d < c.D; ++d) {
    c.secrets.push_back(0x0123456789ABCDEFULL + d);
    c.secrets.push_back(~0ULL - 17 * d);
    c.secrets.push_back(0x8000000000000000ULL | d);
    c.secrets.push_back(d + 1);
  }
  std::vector<Seed> seeds(c.D);
  for (size_t d = 0; d < c.D; ++d) seeds[d].fill((uint8_t)(0x51 + d));
  const uint32_t n = 12;
  const std::vector<uint64_t> all = shamir_shares_wide(params, c.secrets, c.t, SECP_N, seeds, {}, true);
  for (size_t d = 0; d < c.D; ++d)
    for (uint64_t i : c.idx) c.shares.insert(c.shares.end(), all.begin() + (d * n + i) * 4, all.begin() + (d * n + i + 1) * 4);
  return c;
}

static bool same(const CorrectedWideSecrets& a, const CorrectedWideSecrets& b) {
  return a.secrets == b.secrets && a.nerr == b.nerr && a.col_err == b.col_err && a.err_mask == b.err_mask && a.words == b.words;
}

static int check_reports(const std::shared_ptr<PvwParameters>& params, bool host) {
  Case c = make_case(params);
  CorrectedWideSecrets r = shamir_reconstruct_wide_corrected(params, c.idx, c.shares, c.t, SECP_N, false, host);
  for (uint32_t b : r.nerr) if (b) return 1;
  for (uint32_t b : r.col_err) if (b) return 1;
  for (uint64_t b : r.err_mask) if (b) return 1;
  if (r.secrets != c.secrets || r.words != 1) {
    printf("the secrets differ\n");
    return 1;
  }
  // secret 1: columns 0 and 5 wrong (one inside the first t + 1); secret 3: column 6; secret 4: three wrong columns, one too many
  std::vector<uint64_t> sh = c.shares;
  sh[(1 * c.count + 0) * 4 + 3] ^= 4;
  sh[(1 * c.count + 5) * 4 + 1] ^= 1;
  sh[(3 * c.count + 6) * 4 + 0] += 1;
  for (size_t k : {1, 2, 4}) sh[(4 * c.count + k) * 4 + 2] ^= 0x100;
  r = shamir_reconstruct_wide_corrected(params, c.idx, sh, c.t, SECP_N, false, host);
  std::vector<uint64_t> want = c.secrets;
  for (int k = 0; k < 4; ++k) want[4 * 4 + k] = 0;
  if (r.secrets != want || r.nerr != std::vector<uint32_t>{0, 2, 0, 1, PVW_SHAMIR_UNDECODABLE} ||
      r.col_err != std::vector<uint32_t>{1, 0, 0, 0, 0, 1, 1} || !r.wrong(1, 0) || !r.wrong(1, 5) || !r.wrong(3, 6) || r.wrong(1, 1) ||
      r.err_mask[4] || r.err_mask[0]) {
    printf("wrong shares are not reported where they are\n");
    return 1;
  }
  // party-major: the transposed matrix gives the same report
  std::vector<uint64_t> tr(sh.size());
  for (size_t d = 0; d < c.D; ++d)
    for (size_t k = 0; k < c.count; ++k) memcpy(&tr[(k * c.D + d) * 4], &sh[(d * c.count + k) * 4], 32);
  if (!same(shamir_reconstruct_wide_corrected(params, c.idx, tr, c.t, SECP_N, true, host), r)) {
    printf("the party-major report differs\n");
    return 1;
  }
  if (!host && !same(shamir_reconstruct_wide_corrected(params, c.idx, sh, c.t, SECP_N, false, true), r)) {
    printf("the device report differs from the host's\n");
    return 1;
  }
  bool refused = false;
  try {
    Wide even = SECP_N;
    even[0] -= 1;
    shamir_reconstruct_wide_corrected(params, c.idx, c.shares, c.t, even, false, host);
  } catch (const PvwError&) {
    refused = true;
  }
  return refused ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    const bool host = argc > 1 && !strcmp(argv[1], "host");
    auto params = make_params(12);
    if (check_reports(params, host)) return 1;
    printf(host ? "SHAMIR_WIDE_CORRECTED_CPP_HOST_OK\n" : "SHAMIR_WIDE_CORRECTED_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

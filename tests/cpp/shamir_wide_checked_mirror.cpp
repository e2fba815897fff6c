// Checked reconstruction over a 256-bit prime field through the C++ mirror (pvw_host::shamir_reconstruct_wide_checked,
// shamir_wide_from_limbs_device).
// "host": the plain C++ restatement on a consistent sharing, with one wrong extra and one wrong basis share, no GPU.
// No argument: the same matrix through the device form, compared with the restatement word for word.
// Built by tests/test_shamir_wide_checked_host.py everywhere; the device half is run by tests/test_gpu_shamir_wide_checked.py.
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

static std::vector<Seed> make_seeds(size_t count) {
  std::vector<Seed> seeds(count);
  for (size_t d = 0; d < count; ++d) seeds[d].fill((uint8_t)(0x51 + d));
  return seeds;
}

static std::vector<uint64_t> make_secrets(size_t D) {
  std::vector<uint64_t> s;
  for (size_t d = 0; d < D; ++d) {
    s.push_back(0x0123456789ABCDEFULL + d);
    s.push_back(~0ULL - 17 * d);
    s.push_back(0x8000000000000000ULL | d);
    s.push_back(d + 1);
  }
  return s;
}

struct Case {
  std::vector<uint64_t> idx, shares, secrets;   // shares [D][count][4]
  size_t D, count;
  uint32_t t;
};

// D sharings of degree t over n parties (the host restatement of the dealing end), the columns of `idx` picked out
static Case make_case(const std::shared_ptr<PvwParameters>& params) {
  Case c;
  c.D = 5, c.t = 3;
  c.idx = {9, 0, 7, 3, 5, 11, 2};
  c.count = c.idx.size();
  c.secrets = make_secrets(c.D);
  const uint32_t n = 12;
  const std::vector<uint64_t> all = shamir_shares_wide(params, c.secrets, c.t, SECP_N, make_seeds(c.D), {}, true);
  for (size_t d = 0; d < c.D; ++d)
    for (uint64_t i : c.idx) c.shares.insert(c.shares.end(), all.begin() + (d * n + i) * 4, all.begin() + (d * n + i + 1) * 4);
  return c;
}

static int check_reports(const std::shared_ptr<PvwParameters>& params, bool host) {
  Case c = make_case(params);
  CheckedWideSecrets r = shamir_reconstruct_wide_checked(params, c.idx, c.shares, c.t, SECP_N, false, host);
  for (uint32_t b : r.bad) if (b) return 1;
  for (uint32_t b : r.col_bad) if (b) return 1;
  if (r.secrets != c.secrets) {
    printf("the secrets differ\n");
    return 1;
  }
  // a wrong extra share of secret 2 in column 5: flagged there, the secret stays
  std::vector<uint64_t> sh = c.shares;
  sh[(2 * c.count + 5) * 4 + 1] ^= 1;
  r = shamir_reconstruct_wide_checked(params, c.idx, sh, c.t, SECP_N, false, host);
  if (r.secrets != c.secrets || r.bad[2] != 1 || r.col_bad[5] != 1 || r.bad[0] || r.col_bad[4] || r.col_bad[6]) {
    printf("a wrong extra share is not reported where it is\n");
    return 1;
  }
  // a wrong basis share of secret 1: its secret is wrong and every extra of it is flagged
  sh = c.shares;
  sh[(1 * c.count + 2) * 4 + 3] ^= 4;
  r = shamir_reconstruct_wide_checked(params, c.idx, sh, c.t, SECP_N, false, host);
  if (r.bad[1] != c.count - c.t - 1 || r.bad[0] || std::equal(r.secrets.begin() + 4, r.secrets.begin() + 8, c.secrets.begin() + 4)) {
    printf("a wrong basis share is not reported\n");
    return 1;
  }
  // party-major: the transposed matrix gives the same report
  std::vector<uint64_t> tr(sh.size());
  for (size_t d = 0; d < c.D; ++d)
    for (size_t k = 0; k < c.count; ++k) memcpy(&tr[(k * c.D + d) * 4], &sh[(d * c.count + k) * 4], 32);
  const CheckedWideSecrets q = shamir_reconstruct_wide_checked(params, c.idx, tr, c.t, SECP_N, true, host);
  if (q.secrets != r.secrets || q.bad != r.bad || q.col_bad != r.col_bad) {
    printf("the party-major report differs\n");
    return 1;
  }
  if (!host) {   // the device form against the restatement, word for word
    const CheckedWideSecrets h = shamir_reconstruct_wide_checked(params, c.idx, sh, c.t, SECP_N, false, true);
    if (h.secrets != r.secrets || h.bad != r.bad || h.col_bad != r.col_bad) {
      printf("the device report differs from the host's\n");
      return 1;
    }
  }
  bool refused = false;
  try {
    Wide even = SECP_N;
    even[0] -= 1;
    shamir_reconstruct_wide_checked(params, c.idx, c.shares, c.t, even, false, host);
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
    printf(host ? "SHAMIR_WIDE_CHECKED_CPP_HOST_OK\n" : "SHAMIR_WIDE_CHECKED_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

// Reconstruction with erasures over a 256-bit prime field through the C++ mirror (the overload of
// pvw_host::shamir_reconstruct_wide_corrected with `erased`, and pvw_host::shamir_wide_erasure_mask).
// "host": the plain C++ restatement on a consistent sharing with erased columns full of junk, wrong shares beside them, one row
// with more erasures than redundant columns and one the maskless call gives up on, no GPU.
// No argument: the same matrices through the device form, compared with the restatement word for word.
// Built by tests/test_shamir_wide_erasures_host.py everywhere; the device half is run by tests/test_gpu_shamir_wide_erasures.py.
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

static Case make_case(const std::shared_ptr<PvwParameters>& params) {
  Case c;
  c.D = 5, c.t = 2;
  c.idx = {9, 0, 7, 3, 5, 11, 2};                // r = 4
  c.count = c.idx.size();
  for (size_t d = 0; d < c.D; ++d) {
    c.secrets.push_back(0x0123456789ABCDEFULL + d);
    c.secrets.push_back(~0ULL - 17 * d);
    c.secrets.push_back(0x8000000000000000ULL | d);
    c.secrets.push_back(d + 1);
  }
  std::vector<Seed> seeds(c.D);
  for (size_t d = 0; d < c.D; ++d) seeds[d].fill((uint8_t)(0x61 + d));
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
  // an empty mask is the call without one
  if (!same(shamir_reconstruct_wide_corrected(params, c.idx, c.shares, c.t, SECP_N, {}, false, host),
            shamir_reconstruct_wide_corrected(params, c.idx, c.shares, c.t, SECP_N, false, host))) {
    printf("an empty mask changes the report\n");
    return 1;
  }
  // secret 0: four erasures (r of them, no error); secret 1: two erasures and one error; secret 2: nothing; secret 3: three
  // erasures and one error, one column too many; secret 4: five erasures, more than r
  std::vector<uint64_t> sh = c.shares, erased(c.D, 0);
  auto erase = [&](size_t s, size_t k) {
    erased[s] |= 1ULL << k;
    for (int w = 0; w < 4; ++w) sh[(s * c.count + k) * 4 + w] = ~0ULL;   // 2^256 - 1: nothing there is read
  };
  for (size_t k : {0, 2, 3, 6}) erase(0, k);
  for (size_t k : {1, 5}) erase(1, k);
  sh[(1 * c.count + 0) * 4 + 3] ^= 4;
  for (size_t k : {0, 1, 4}) erase(3, k);
  sh[(3 * c.count + 6) * 4 + 0] += 1;
  for (size_t k : {0, 1, 2, 3, 4}) erase(4, k);
  erased[2] = ~0ULL << c.count;                  // padding bits are ignored
  CorrectedWideSecrets r = shamir_reconstruct_wide_corrected(params, c.idx, sh, c.t, SECP_N, erased, false, host);
  std::vector<uint64_t> want = c.secrets;
  for (int k = 0; k < 4; ++k) want[3 * 4 + k] = want[4 * 4 + k] = 0;
  if (r.secrets != want || r.nerr != std::vector<uint32_t>{0, 1, 0, PVW_SHAMIR_UNDECODABLE, PVW_SHAMIR_UNDECODABLE} ||
      r.col_err != std::vector<uint32_t>{1, 0, 0, 0, 0, 0, 0} || r.err_mask != std::vector<uint64_t>{0, 1, 0, 0, 0}) {
    printf("the report with erasures is not what was planted\n");
    return 1;
  }
  // the maskless call gives up on secret 0 (four junk columns, E = 2)
  if (shamir_reconstruct_wide_corrected(params, c.idx, sh, c.t, SECP_N, false, host).nerr[0] != PVW_SHAMIR_UNDECODABLE) {
    printf("four junk columns decode without a mask\n");
    return 1;
  }
  // party-major: the transposed matrix gives the same report (the mask stays [secret][word])
  std::vector<uint64_t> tr(sh.size());
  for (size_t d = 0; d < c.D; ++d)
    for (size_t k = 0; k < c.count; ++k) memcpy(&tr[(k * c.D + d) * 4], &sh[(d * c.count + k) * 4], 32);
  if (!same(shamir_reconstruct_wide_corrected(params, c.idx, tr, c.t, SECP_N, erased, true, host), r)) {
    printf("the party-major report differs\n");
    return 1;
  }
  if (!host && !same(shamir_reconstruct_wide_corrected(params, c.idx, sh, c.t, SECP_N, erased, false, true), r)) {
    printf("the device report differs from the host's\n");
    return 1;
  }
  // the mask from a per-limb report: NL = 5, a share is erased as soon as one limb is flagged
  const uint32_t NL = 5;
  std::vector<uint32_t> status(c.D * c.count * NL, 0);
  std::vector<uint64_t> noise(c.D * c.count * NL, 3);
  status[(0 * c.count + 2) * NL + 4] = 1;
  noise[(1 * c.count + 5) * NL + 0] = 1000;
  noise[(1 * c.count + 6) * NL + 2] = 10;        // == the bound: not flagged
  const std::vector<uint64_t> mask = shamir_wide_erasure_mask(status, noise, c.count, NL, 1, 10);
  if (mask != std::vector<uint64_t>{4, 32, 0, 0, 0}) {
    printf("the mask of the per-limb report is wrong\n");
    return 1;
  }
  bool refused = false;
  try {
    shamir_reconstruct_wide_corrected(params, c.idx, c.shares, c.t, SECP_N, std::vector<uint64_t>(3, 0), false, host);
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
    printf(host ? "SHAMIR_WIDE_ERASURES_CPP_HOST_OK\n" : "SHAMIR_WIDE_ERASURES_CPP_OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

// Checked reconstruction through the C++ mirror (pvw_host::shamir_reconstruct_checked).
// "host": the plain restatement, no GPU -- a clean sharing, one bent extra, one bent basis share, both layouts, a refusal.
// No argument: the same report from the device, and the loop closed: deal -> every party's aggregate share -> the checked sum.
// Built by tests/test_shamir_check_host.py everywhere; the device half is run by tests/test_gpu_shamir_check.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

static const uint64_t P61 = (1ULL << 61) - 1;

static std::vector<Seed> make_seeds(size_t D) {
  std::vector<Seed> seeds(D);
  for (size_t d = 0; d < D; ++d) seeds[d].fill((uint8_t)(0x61 + d));
  return seeds;
}

static bool same(const CheckedSecrets& a, const CheckedSecrets& b) {
  return a.secrets == b.secrets && a.bad == b.bad && a.col_bad == b.col_bad;
}

// the cases of both halves: shares [D][n] of a degree-t sharing, all n columns in a scrambled order
struct Cases {
  uint32_t n, t;
  std::vector<uint64_t> secrets, idx, picked;   // picked [D][n] in the order of idx
  size_t D;
};
static Cases make_cases(const std::shared_ptr<PvwParameters>& params, uint32_t n, uint32_t t) {
  Cases c{n, t, {5, ~0ULL, P61 + 3}, {}, {}, 3};
  const std::vector<uint64_t> shares = shamir_shares(params, c.secrets, t, P61, make_seeds(c.D), {}, true);
  for (uint32_t i = 0; i < n; ++i) c.idx.push_back((i * 5 + 3) % n);   // n = 12: 5 is a unit, so a permutation
  for (size_t d = 0; d < c.D; ++d)
    for (uint64_t i : c.idx) c.picked.push_back(shares[d * n + i]);
  return c;
}

static int run_cases(const std::shared_ptr<PvwParameters>& params, const Cases& c, bool host) {
  const uint32_t n = c.n, t = c.t;
  const size_t D = c.D;
  CheckedSecrets r = shamir_reconstruct_checked(params, c.idx, c.picked, t, P61, host);
  for (size_t d = 0; d < D; ++d)
    if (r.secrets[d] != c.secrets[d] % P61 || r.bad[d] != 0) return 1;
  for (uint32_t v : r.col_bad)
    if (v != 0) return 2;
  // party-major: the transposed matrix gives the same report
  std::vector<uint64_t> tr(c.picked.size());
  for (size_t d = 0; d < D; ++d)
    for (size_t i = 0; i < n; ++i) tr[i * D + d] = c.picked[d * n + i];
  if (!same(shamir_reconstruct_checked(params, c.idx, tr, t, P61, host, true), r)) return 3;
  // one bent extra: exactly that place
  std::vector<uint64_t> bent = c.picked;
  bent[1 * n + (t + 2)] ^= 1;
  r = shamir_reconstruct_checked(params, c.idx, bent, t, P61, host);
  for (size_t d = 0; d < D; ++d)
    if (r.secrets[d] != c.secrets[d] % P61 || r.bad[d] != (d == 1 ? 1u : 0u)) return 4;
  for (size_t i = 0; i < n; ++i)
    if (r.col_bad[i] != (i == t + 2 ? 1u : 0u)) return 5;
  // one bent basis share: the secret is wrong and every extra of it deviates
  bent = c.picked;
  bent[2 * n + 1] += 1;
  r = shamir_reconstruct_checked(params, c.idx, bent, t, P61, host);
  if (r.secrets[2] == c.secrets[2] % P61 || r.bad[2] != n - t - 1 || r.bad[0] != 0 || r.bad[1] != 0) return 6;
  for (size_t i = 0; i < n; ++i)
    if (r.col_bad[i] != (i > t ? 1u : 0u)) return 7;
  // host and device agree on it
  if (!host && !same(r, shamir_reconstruct_checked(params, c.idx, bent, t, P61, true))) return 8;
  bool refused = false;
  try {
    std::vector<uint64_t> dup = c.idx;
    dup[3] = dup[0];
    shamir_reconstruct_checked(params, dup, c.picked, t, P61, host);
  } catch (const PvwError&) {
    refused = true;
  }
  return refused ? 0 : 9;
}

static int host_half() {
  const uint32_t n = 12, t = 4;
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const int rc = run_cases(params, make_cases(params, n, t), true);
  if (rc) {
    printf("host case %d failed\n", rc);
    return 1;
  }
  printf("RECONSTRUCT_CPP_HOST_OK\n");
  return 0;
}

static int device_half() {
  const std::vector<uint64_t> moduli = {0x800000022A0001ULL, 0x800000021A0001ULL, 0x80000002120001ULL, 0x80000001F60001ULL};
  const uint32_t n = 12, t = 4;
  auto params = PvwParametersBuilder().set_parties(n).set_dimension(4).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const Cases c = make_cases(params, n, t);
  const int rc = run_cases(params, c, false);
  if (rc) {
    printf("device case %d failed\n", rc);
    return 1;
  }
  // the loop closed: every party's aggregate share of the dealt secrets, all n of them checked against the first t + 1
  Seed seed;
  seed.fill(0x3D);
  PvwCrs crs = PvwCrs::new_deterministic(params, seed);
  GlobalPublicKey global_pk(crs);
  std::vector<Party> parties;
  for (uint32_t i = 0; i < n; ++i) parties.push_back(Party::create(i, params, seed));
  global_pk.generate_all_party_keys(parties, seed);
  auto cts = deal_party_shares(c.secrets, t, P61, global_pk, make_seeds(c.D));
  const pvw_plain_t plain{P61, 0, nullptr};
  CheckedShares sums = decrypt_all_party_sums(cts, parties, {}, 0, &plain);
  std::vector<uint64_t> natural;
  for (uint32_t i = 0; i < n; ++i) natural.push_back(i);
  uint64_t want = 0;
  for (uint64_t v : c.secrets) want = (want + v % P61) % P61;
  CheckedSecrets r = shamir_reconstruct_checked(params, natural, sums.values, t, P61);
  if (r.secrets[0] != want || r.bad[0] != 0) {
    printf("sum %llu (bad %u), expected %llu\n", (unsigned long long)r.secrets[0], r.bad[0], (unsigned long long)want);
    return 1;
  }
  // one party reports a wrong sum: its column is flagged
  sums.values[n - 2] ^= 4;
  r = shamir_reconstruct_checked(params, natural, sums.values, t, P61);
  if (r.secrets[0] != want || r.bad[0] != 1 || r.col_bad[n - 2] != 1) return 1;
  printf("RECONSTRUCT_CPP_OK\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    return argc > 1 && !strcmp(argv[1], "host") ? host_half() : device_half();
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
}

// The wide handover through the C++ mirror (pvw_host::shamir_wide_handover_shape, shamir_wide_signed_digits,
// shamir_wide_handover_weights, shamir_wide_from_digits, shamir_packed_wide_handover_points, wide_handover_fits,
// decrypt_all_party_handover_wide).  "host": the public pieces on values whose digits are known by hand, the
// advisory fit and a refusal; no GPU.
// Built and run by tests/test_shamir_wide_handover_host.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

// the order of the secp256k1 group
static const Wide SECP_N = {0xBFD25E8CD0364141ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, 0xFFFFFFFFFFFFFFFFULL};

#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      return 1;                                                 \
    }                                                           \
  } while (0)

static int host_half() {
  const WideHandoverShape s = shamir_wide_handover_shape(SECP_N, 52, 52);
  EXPECT(s.num_limbs == 5 && s.num_digits == 5);                                  // ceil(256 / 52), ceil(257 / 52)
  EXPECT(shamir_wide_handover_shape(SECP_N, 52, 64).num_digits == 5 && shamir_wide_handover_shape(SECP_N, 62, 8).num_digits == 33);
  // 1 -> (1, 0, ..), p - 1 -> (-1, 0, ..), p -> 0
  std::vector<uint64_t> vals = {1, 0, 0, 0, SECP_N[0] - 1, SECP_N[1], SECP_N[2], SECP_N[3], SECP_N[0], SECP_N[1], SECP_N[2], SECP_N[3]};
  const std::vector<int64_t> dg = shamir_wide_signed_digits(vals, SECP_N, 64);
  EXPECT(dg.size() == 15 && dg[0] == 1 && dg[5] == -1);
  for (size_t i = 0; i < 15; ++i) EXPECT(i == 0 || i == 5 || dg[i] == 0);
  // one holder: lambda = 1, so limb w's weight is 2^(52 w), whose digits in base 2^52 are the unit vector of w
  const std::vector<int64_t> w = shamir_wide_handover_weights({3}, SECP_N, {}, {}, 52, 52);
  EXPECT(w.size() == 25);
  for (size_t v = 0; v < 5; ++v)
    for (size_t l = 0; l < 5; ++l) EXPECT(w[v * 5 + l] == (v == l ? 1 : 0));
  // a masked holder's columns are 0; a point on the valid holder gives its unit vector again
  const std::vector<int64_t> w2 = shamir_wide_handover_weights({3, 8}, SECP_N, {false, true}, {9, 0, 0, 0}, 52, 52);
  EXPECT(w2.size() == 50);
  for (size_t v = 0; v < 5; ++v)
    for (size_t l = 0; l < 5; ++l) EXPECT(w2[v * 10 + l] == 0 && w2[v * 10 + 5 + l] == (v == l ? 1 : 0));
  const std::vector<uint64_t> pts = shamir_packed_wide_handover_points(SECP_N, 3);
  EXPECT(pts.size() == 12 && pts[0] == 0 && pts[3] == 0 && pts[4] == SECP_N[0] - 1 && pts[8] == SECP_N[0] - 2 && pts[11] == SECP_N[3]);
  // -3 + 5 2^16, the sign bit dropped from the status and the others kept
  const WideHandoverShares f = shamir_wide_from_digits({3, 5}, {PVW_DEC_NEGATIVE | PVW_DEC_WIDE_TRUNCATED, PVW_DEC_LOSSY}, 2, 1, SECP_N, 16);
  EXPECT(f.values.size() == 4 && f.values[0] == (5u << 16) - 3 && f.values[1] == 0 && f.values[3] == 0);
  EXPECT(f.status.size() == 1 && f.status[0] == (PVW_DEC_WIDE_TRUNCATED | PVW_DEC_LOSSY));
  const std::vector<uint64_t> moduli = {0xFFFFEE001ULL, 0xFFFFC4001ULL, 0x1FFFFE0001ULL};
  auto params = PvwParametersBuilder().set_parties(12).set_dimension(2).set_l(8).set_moduli(moduli)
                    .set_secret_variance(0.5f).set_error_bounds_u32(100, 200).build_arc();
  const bool fits = wide_handover_fits(params, SECP_N, 5, 52, 64);
  EXPECT(fits == lincomb_fits(params, std::vector<int64_t>(25, INT64_MIN)));      // 110 bits of Q hold the 123-bit plaintexts in 2 words
  bool refused = false;
  try {
    shamir_wide_handover_weights({3, 3}, SECP_N);                                  // a duplicate holder
  } catch (const PvwError& e) {
    refused = e.code == 1;
  }
  EXPECT(refused);
  printf("SHAMIR_WIDE_HANDOVER_CPP_HOST_OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "host")) return host_half();
  fprintf(stderr, "usage: %s host\n", argv[0]);
  return 2;
}

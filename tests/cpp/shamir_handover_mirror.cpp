// The one-word handover through the C++ mirror (pvw_host::shamir_handover_weights, shamir_valid_mask,
// decrypt_all_party_handover).  "host": the weights on cases whose values are known by hand, the mask of a
// small report and a refusal; no GPU.
// Built and run by tests/test_shamir_handover_host.py.
#include <cstdio>
#include <cstring>

#include "../../pvw_rs_amd/host/pvw.hpp"

using namespace pvw_host;

#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      return 1;                                                 \
    }                                                           \
  } while (0)

static int host_half() {
  const uint64_t p = 65537;
  // the points 1 and 2 at 0: L_1(0) = 2, L_2(0) = -1
  const HandoverWeights a = shamir_handover_weights({0, 1}, p);
  EXPECT(a.count == 2 && a.weights.size() == 2 && a.weights[0] == 2 && a.weights[1] == -1);
  // the middle holder masked: its column is 0 and the others are the weights of the points 1 and 3 at 0: 3/2 and -1/2
  const HandoverWeights b = shamir_handover_weights({0, 1, 2}, p, {true, false, true});
  const std::vector<std::vector<int64_t>> ref = shamir_lagrange_weights_at({0, 2}, {p - 1}, p);
  EXPECT(b.count == 2 && b.weights[0] == ref[0][0] && b.weights[1] == 0 && b.weights[2] == ref[0][1]);
  // a target on a valid holder is its unit vector; on the masked holder it is an ordinary point; p - 2 is the point -1
  const HandoverWeights c = shamir_handover_weights({0, 1, 2}, p, {true, false, true}, {2, 1, p - 2});
  const std::vector<std::vector<int64_t>> rc = shamir_lagrange_weights_at({0, 2}, {2, 1, p - 2}, p);
  EXPECT(c.weights.size() == 9 && c.weights[0] == 0 && c.weights[1] == 0 && c.weights[2] == 1);
  for (size_t j = 0; j < 3; ++j) EXPECT(c.weights[j * 3] == rc[j][0] && c.weights[j * 3 + 1] == 0 && c.weights[j * 3 + 2] == rc[j][1]);
  EXPECT((c.weights[3] + c.weights[5] - 1) % (int64_t)p == 0);                     // the weights of a row add up to 1 mod p
  // nobody valid: zeros and count 0, no error
  const HandoverWeights z = shamir_handover_weights({0, 1}, p, {false, false});
  EXPECT(z.count == 0 && z.weights[0] == 0 && z.weights[1] == 0);
  // the mask of a [2][3] report: column 1 has a status bit in row 1, column 2 a noise above the bound in row 0
  const ValidMask m = shamir_valid_mask({0, 0, 0, 0, 4, 0}, {1, 2, 9, 1, 2, 3}, 3, 0xFFFFFFFFu, 8);
  EXPECT(m.num_valid == 1 && m.valid[0] == 1 && m.valid[1] == 0 && m.valid[2] == 0);
  const ValidMask m2 = shamir_valid_mask({0, 0, 0, 0, 4, 0}, {}, 3, 3);            // bit 2 is not asked for
  EXPECT(m2.num_valid == 3);
  bool refused = false;
  try {
    shamir_handover_weights({3, 3}, p, {true, false});                             // a duplicate, although one of them is masked
  } catch (const PvwError& e) {
    refused = e.code == 1;
  }
  EXPECT(refused);
  printf("SHAMIR_HANDOVER_CPP_HOST_OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "host")) return host_half();
  fprintf(stderr, "usage: %s host\n", argv[0]);
  return 2;
}

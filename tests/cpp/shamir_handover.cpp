// The masked product chain of the one-word handover weights (pvw_rs_amd/csrc/pvw_shamir.hip), restated sequentially
// in the kernels' order over pvw_arith.h: the mask bytes 64 at a time as a ballot, u_i = (prod over the valid k != i of
// (x_i - x_k))^-1 with the 64 lanes' partial products met by xor shuffles and 0 for a masked i (shamir_masked_prod_kernel), the
// scale and the coinciding VALID column of every target (shamir_masked_target_scale_kernel), the Cauchy entries over ALL columns
// with SH_CB differences per Fermat inversion (shamir_cauchy_kernel), then lambda = scale C or the unit row, centred
// (shamir_handover_weights_kernel), and the count of the mask bytes.  The program prints what the kernels would store; the test
// compares it with pvw_shamir_handover_weights_host, which runs prefix and suffix products over the compacted holders instead.
// Stand-alone: shamir_handover <p> <mask of 0/1 characters, or - for none> <index,index,..> <target,target,..>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pvw_arith.h"

using namespace pvw;

static const u32 NO_COLUMN = 0xFFFFFFFFu, CB = 8;

static std::vector<u64> parse_list(const char* s) {
  std::vector<u64> out;
  while (*s) {
    char* end;
    out.push_back(strtoull(s, &end, 10));
    s = *end == ',' ? end + 1 : end;
  }
  return out;
}

// the ballot of the 64 holders from c0 on; valid == NULL is everybody
static u64 ballot(const std::vector<unsigned char>* valid, u32 c0, u32 count) {
  u64 b = 0;
  for (u32 lane = 0; lane < 64; ++lane)
    if (c0 + lane < count && (!valid || (*valid)[c0 + lane] != 0)) b |= (u64)1 << lane;
  return b;
}
// wave_mulmod: every lane ends with the product of all 64
static u64 meet(u64 (&v)[64], const Mod& m) {
  for (u32 off = 32; off; off >>= 1) {
    u64 nv[64];
    for (u32 l = 0; l < 64; ++l) nv[l] = mulmod(v[l], v[l ^ off], m);
    memcpy(v, nv, sizeof v);
  }
  return v[0];
}
static u64 inv(u64 a, const Mod& m) { return powmod(a, m.q - 2, m); }

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const u64 p = strtoull(argv[1], nullptr, 10);
  const Mod m = make_mod(p);
  const std::vector<u64> idx = parse_list(argv[3]), tgt = parse_list(argv[4]);
  const u32 D = (u32)idx.size(), T = (u32)tgt.size();
  std::vector<unsigned char> mask;
  const bool all = !strcmp(argv[2], "-");
  if (!all) {
    if (strlen(argv[2]) != D) return 2;
    for (u32 d = 0; d < D; ++d) mask.push_back(argv[2][d] == '1' ? 0x80 : 0);   // any byte that is not 0 is valid
  }
  const std::vector<unsigned char>* valid = all ? nullptr : &mask;
  std::vector<u64> x(D), xt(T), aux(D), scale(T), C((size_t)D * T);
  std::vector<u32> coin(T);
  std::vector<i64> W((size_t)T * D);
  for (u32 i = 0; i < D; ++i) x[i] = idx[i] + 1;                      // shamir_points_kernel
  for (u32 j = 0; j < T; ++j) xt[j] = tgt[j] + 1;                     // the target p - 1 becomes p: submod takes it as 0
  for (u32 i = 0; i < D; ++i) {                                       // shamir_masked_prod_kernel, one wave per holder
    const u64 own = ballot(valid, i & ~63u, D);
    if (!((own >> (i & 63)) & 1)) {
      aux[i] = 0;
      continue;
    }
    u64 prod[64];
    for (u32 l = 0; l < 64; ++l) prod[l] = 1;
    for (u32 c0 = 0; c0 < D; c0 += 64) {
      const u64 bal = ballot(valid, c0, D);
      if (!bal) continue;
      for (u32 l = 0; l < 64; ++l)
        if (((bal >> l) & 1) && c0 + l != i) prod[l] = mulmod(prod[l], submod(x[i], x[c0 + l], m.q), m);
    }
    aux[i] = inv(meet(prod, m), m);
  }
  u32 count = 0;                                                      // shamir_valid_count_kernel
  for (u32 c0 = 0; c0 < D; c0 += 64) count += (u32)__builtin_popcountll(ballot(valid, c0, D));
  for (u32 j = 0; j < T; ++j) {                                       // shamir_masked_target_scale_kernel, one wave per target
    u64 prod[64];
    u32 hit[64];
    for (u32 l = 0; l < 64; ++l) prod[l] = 1, hit[l] = NO_COLUMN;
    for (u32 c0 = 0; c0 < D; c0 += 64) {
      const u64 bal = ballot(valid, c0, D);
      if (!bal) continue;
      for (u32 l = 0; l < 64; ++l)
        if ((bal >> l) & 1) {
          const u64 d = submod(xt[j], x[c0 + l], m.q);
          if (d == 0) hit[l] = c0 + l;
          else prod[l] = mulmod(prod[l], d, m);
        }
    }
    scale[j] = meet(prod, m);
    u32 h = NO_COLUMN;
    for (u32 l = 0; l < 64; ++l) h = hit[l] < h ? hit[l] : h;
    coin[j] = h;
  }
  for (u32 i0 = 0; i0 < D; i0 += CB)                                  // shamir_cauchy_kernel: a thread owns one target and CB columns
    for (u32 j = 0; j < T; ++j) {
      u64 d[CB], pre[CB], run = 1;
      for (u32 b = 0; b < CB; ++b) {
        const u32 i = i0 + b;
        d[b] = i < D ? submod(xt[j], x[i], m.q) : 0;
        pre[b] = run;
        run = mulmod(run, d[b] ? d[b] : 1, m);
      }
      u64 iv = inv(run, m);
      for (u32 b = CB; b-- > 0;) {
        const u32 i = i0 + b;
        const u64 di = mulmod(iv, pre[b], m);
        iv = mulmod(iv, d[b] ? d[b] : 1, m);
        if (i < D) C[(size_t)i * T + j] = d[b] ? mulmod(aux[i], di, m) : 0;
      }
    }
  for (size_t e = 0; e < (size_t)D * T; ++e) {                        // shamir_handover_weights_kernel, the holder fastest
    const u32 i = (u32)(e % D), j = (u32)(e / D);
    const u32 c = coin[j];
    const u64 lam = c != NO_COLUMN ? (c == i ? 1 : 0) : mulmod(scale[j], C[(size_t)i * T + j], m);
    W[e] = lam > m.q / 2 ? -(i64)(m.q - lam) : (i64)lam;
  }
  printf("C %u\nW", count);
  for (size_t e = 0; e < W.size(); ++e) printf(" %" PRId64, (int64_t)W[e]);
  printf("\nSHAMIR_HANDOVER_OK\n");
  return 0;
}

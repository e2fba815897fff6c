// Packed dealing over a prime below 2^256 (pvw_rs_amd/csrc/pvw_shamir.hip), restated sequentially in the kernels'
// own order and forms over pvw_wide.h: the basis kernel (one inversion of (K-1)!, the walk down, w_j R^3), the weights kernel
// (suffix and prefix passes by wide_step, two Montgomery products an entry, Z(x) in full) and the packed evaluation (Horner over
// a_t .. a_1, the unreduced accumulator started on R(x) zt, K products added, one reduction) -- against the definition computed
// another way: every L_j(x) from its own factors over separately inverted differences, powers of x by repeated products, all
// in Montgomery form with fully reduced additions.  Stand-alone: shamir_packed_wide <cases per prime> <prime in hex>...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvw_wide.h"

using namespace pvw;

struct W4 {
  u64 v[4];
};

static u64 rng_state;
static u64 rnd64() {   // splitmix64
  u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static bool parse_hex(const char* h, u64 (&out)[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  const size_t len = strlen(h);
  if (len == 0 || len > 64) return false;
  for (size_t i = 0; i < len; ++i) {
    const char ch = h[len - 1 - i];
    u64 dgt;
    if (ch >= '0' && ch <= '9') dgt = (u64)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') dgt = (u64)(ch - 'a' + 10);
    else return false;
    out[i / 16] |= dgt << (4 * (i % 16));
  }
  return true;
}

static W4 small(u64 v) { return W4{{v, 0, 0, 0}}; }
static W4 mmul(const W4& a, const W4& b, const WideMont& m) {
  W4 r;
  wide_mont_mul(a.v, b.v, m, r.v);
  return r;
}
static W4 mul(const W4& a, const W4& b, const WideMont& m) {   // a b mod p
  W4 r;
  wide_mul(a.v, b.v, m, r.v);
  return r;
}
static W4 min_(const W4& a, const WideMont& m) {   // a R mod p for any words
  W4 r;
  wide_mont_in(a.v, m, r.v);
  return r;
}
static W4 mout(const W4& a, const WideMont& m) {
  W4 r;
  wide_mont_out(a.v, m, r.v);
  return r;
}

// ---- the kernels, sequentially ------------------------------------------------------------------------------------------
static void basis(std::vector<W4>& w3, u32 K, const WideMont& mm) {
  std::vector<W4> invf(K);
  W4 f;
  memcpy(f.v, mm.one, 32);
  for (u32 j = 2; j < K; ++j) f = mul(small(j), f, mm);
  W4 inv;
  wide_mont_inv(f.v, mm, inv.v);
  for (u32 j = K - 1;; --j) {
    invf[j] = inv;
    if (j == 0) break;
    inv = mul(small(j), inv, mm);
  }
  w3.resize(K);
  for (u32 j = 0; j < K; ++j) {
    W4 a = mmul(invf[j], invf[K - 1 - j], mm);
    if (j & 1) {
      W4 z = small(0);
      wide_sub_p(z.v, a.v, mm);
      a = z;
    }
    W4 r2;
    memcpy(r2.v, mm.r2, 32);
    a = mmul(a, r2, mm);
    a = mmul(a, r2, mm);
    w3[j] = a;
  }
}

static void weights(std::vector<W4>& Lw, W4& zt, const std::vector<W4>& w3, u32 K, u32 x, const WideMod& m, const WideMont& mm) {
  const u64 zero[4] = {0, 0, 0, 0};
  Lw.resize(K);
  u64 suf[4] = {1, 0, 0, 0};
  wide_shl(suf, m.shift);
  for (u32 j = K; j-- > 0;) {
    memcpy(Lw[j].v, suf, 32);
    wide_step(suf, x + j, zero, m);
  }
  wide_shr(suf, m.shift);
  wide_mont_in(suf, mm, zt.v);
  u64 pre[4] = {1, 0, 0, 0};
  wide_shl(pre, m.shift);
  for (u32 j = 0; j < K; ++j) {
    W4 sv = Lw[j], pv;
    wide_shr(sv.v, m.shift);
    memcpy(pv.v, pre, 32);
    wide_shr(pv.v, m.shift);
    sv = mmul(sv, pv, mm);
    Lw[j] = mmul(sv, w3[j], mm);
    wide_step(pre, x + j, zero, m);
  }
}

static W4 eval_packed(const std::vector<W4>& secrets, const std::vector<W4>& coeffs, const std::vector<W4>& Lw, const W4& zt, u32 x,
                      const WideMod& m, const WideMont& mm) {
  const u32 t = (u32)coeffs.size(), K = (u32)secrets.size();
  u64 acc[4] = {0, 0, 0, 0};
  for (u32 e = t; e >= 1; --e) {
    u64 a[4];
    wide_reduce_scaled(coeffs[e - 1].v, m, a);
    wide_step(acc, x, a, m);
  }
  wide_shr(acc, m.shift);
  u32 T[16], P[16];
  wide_mul_full(acc, zt.v, T);
  for (u32 j = 0; j < K; ++j) {
    u64 s[4];
    wide_reduce_scaled(secrets[j].v, m, s);
    wide_shr(s, m.shift);
    wide_mul_full(s, Lw[j].v, P);
    wide_acc_add(T, P, mm);
  }
  W4 out;
  wide_redc(T, mm, out.v);
  return out;
}

// ---- the definition, another way (Montgomery form throughout) ---------------------------------------------------------------
// dinv[d] = R / d for 0 < d < K, each by its own Fermat inversion
static std::vector<W4> difference_inverses(u32 K, const WideMont& mm) {
  std::vector<W4> dinv(K);
  for (u32 d = 1; d < K; ++d) {
    const W4 dm = min_(small(d), mm);
    wide_mont_inv(dm.v, mm, dinv[d].v);
  }
  return dinv;
}
static W4 definition(const std::vector<W4>& secrets, const std::vector<W4>& coeffs, const std::vector<W4>& dinv, u32 x, const WideMont& mm) {
  const u32 t = (u32)coeffs.size(), K = (u32)secrets.size();
  W4 one;
  memcpy(one.v, mm.one, 32);
  W4 acc = small(0);
  const W4 xm = min_(small(x), mm);
  for (u32 j = 0; j < K; ++j) {
    W4 l = one;
    for (u32 mth = 0; mth < K; ++mth) {
      if (mth == j) continue;
      // (x + mth) / (mth - j): the points are -j and -mth
      W4 inv = dinv[mth > j ? mth - j : j - mth];
      if (mth < j) {
        W4 z = small(0);
        wide_sub_p(z.v, inv.v, mm);
        inv = z;
      }
      l = mmul(mmul(l, min_(small((u64)x + mth), mm), mm), inv, mm);
    }
    const W4 term = mmul(min_(secrets[j], mm), l, mm);
    wide_add_p(acc.v, term.v, mm);
  }
  W4 Z = one;
  for (u32 mth = 0; mth < K; ++mth) Z = mmul(Z, min_(small((u64)x + mth), mm), mm);
  W4 r = small(0), pw = one;
  for (u32 e = 0; e < t; ++e) {
    const W4 term = mmul(min_(coeffs[e], mm), pw, mm);
    wide_add_p(r.v, term.v, mm);
    pw = mmul(pw, xm, mm);
  }
  const W4 zr = mmul(Z, r, mm);
  wide_add_p(acc.v, zr.v, mm);
  return mout(acc, mm);
}

static W4 edge_word(const u64 (&p)[4], u32 i) {
  W4 w;
  switch (i % 5) {
    case 0: return small(0);
    case 1: memcpy(w.v, p, 32); w.v[0] -= 1; return w;          // p - 1 (p odd)
    case 2: memcpy(w.v, p, 32); return w;                       // p
    case 3: w.v[0] = w.v[1] = w.v[2] = w.v[3] = ~(u64)0; return w;
    default: for (int k = 0; k < 4; ++k) w.v[k] = rnd64(); return w;
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: shamir_packed_wide <cases per prime> <prime in hex>...\n");
    return 2;
  }
  const u32 cases = (u32)atoi(argv[1]);
  for (int a = 2; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p)) {
      fprintf(stderr, "bad prime %s\n", argv[a]);
      return 2;
    }
    const WideMod m = make_wide_mod(p);
    const WideMont mm = make_wide_mont(p);
    rng_state = p[0] ^ 0x5eed;
    static const u32 PACKS[] = {1, 2, 3, 5, 8, 17};
    static const u32 XS[] = {1, 2, 255, 4096, 65000};                 // x + K - 1 < 65537
    // a prime below 65537 serves the packs and points with x + K - 1 < p only: the others are left out, and the last point is
    // the largest one the pack leaves, x = p - K
    const bool small_p = !(p[1] | p[2] | p[3]) && p[0] < 65537;
    u32 served = 0;
    for (u32 c = 0; c < cases; ++c) {
      const u32 K = PACKS[c % 6], t = (c / 6) % 5;
      if (small_p && (u64)K + 1 > p[0]) continue;                        // not even x = 1
      ++served;
      std::vector<W4> w3;
      basis(w3, K, mm);
      const std::vector<W4> dinv = difference_inverses(K, mm);
      std::vector<W4> secrets(K), coeffs(t);
      for (u32 j = 0; j < K; ++j) secrets[j] = edge_word(p, c + j);
      for (u32 j = 0; j < t; ++j) coeffs[j] = edge_word(p, c + j + 2);
      for (u32 xi = 0; xi < 5; ++xi) {
        u32 x = XS[xi];
        if (small_p && xi == 4) x = (u32)p[0] - K;
        if (small_p && (u64)x + K > p[0]) continue;
        std::vector<W4> Lw;
        W4 zt;
        weights(Lw, zt, w3, K, x, m, mm);
        const W4 got = eval_packed(secrets, coeffs, Lw, zt, x, m, mm), want = definition(secrets, coeffs, dinv, x, mm);
        if (memcmp(got.v, want.v, 32) != 0 || !wide_less(got.v, p)) {
          printf("MISMATCH prime %s K %u t %u x %u\n", argv[a], K, t, x);
          return 1;
        }
      }
    }
    if (!served) {
      printf("prime %s served no case\n", argv[a]);
      return 1;
    }
  }
  printf("SHAMIR_PACKED_WIDE_OK\n");
  return 0;
}

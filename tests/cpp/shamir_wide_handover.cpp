// The public arithmetic of the wide handover (pvw_rs_amd/csrc/pvw_shamir.hip), restated sequentially in the kernels'
// order and Montgomery forms over pvw_wide.h: the points of the valid holders and of the targets times R, the column weights u_i
// (one wave per product, the 64 partial products met in lane 0, Fermat's inversion), the scale and coinciding column of every
// target met over 64 lanes, the Cauchy entries with 32 differences per inversion, then shamir_handover_digits_wide_kernel
// (lambda = scale C or the unit vector, one product by 2^limb_bits R per limb, out of Montgomery form, centred, cut),
// shamir_signed_digits_wide_kernel and shamir_wide_from_digits_kernel.  The program prints what the kernels would store; the
// test compares it with the _host routines of the library, which run the scaled step and prefix / suffix products instead.
// Stand-alone: shamir_wide_handover [holders=i,j,..] <prime in hex>...
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvw_wide.h"

using namespace pvw;

struct W4 {
  u64 v[4];
};
static const u32 NO_COLUMN = 0xFFFFFFFFu, BATCH = 32, DEC_NEGATIVE = 2;

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

static bool is0(const W4& a) { return !(a.v[0] | a.v[1] | a.v[2] | a.v[3]); }
static W4 mul(const W4& a, const W4& b, const WideMont& m) {
  W4 r;
  wide_mont_mul(a.v, b.v, m, r.v);
  return r;
}
static W4 sub(W4 a, const W4& b, const WideMont& m) {
  wide_sub_p(a.v, b.v, m);
  return a;
}
static W4 one(const WideMont& m) {
  W4 r;
  memcpy(r.v, m.one, 32);
  return r;
}
static W4 inv(const W4& a, const WideMont& m) {
  W4 r;
  wide_mont_inv(a.v, m, r.v);
  return r;
}
static W4 mont_in(const W4& a, const WideMont& m) {
  W4 r;
  wide_mont_in(a.v, m, r.v);
  return r;
}

// the product of 64 lanes' values as shamir_prod_wide_kernel meets them: lane 0 multiplies the others in, in order
static W4 meet_in_lane0(const W4 (&lane)[64], const WideMont& m) {
  W4 p = lane[0];
  for (u32 i = 1; i < 64; ++i) p = mul(p, lane[i], m);
  return p;
}

// weights [T V][D NL] by the kernels' sequence; x the valid holders' points and xt the targets, plain and below p
static std::vector<i64> kernel_weights(const std::vector<W4>& xp, const std::vector<u32>& col, const std::vector<W4>& xtp, u32 D, u32 NL, u32 V,
                                       u32 limb_bits, u32 b, const WideMont& m) {
  const u32 nv = (u32)xp.size(), T = (u32)xtp.size();
  std::vector<W4> x(nv), xt(T), u(nv), scale(T), C((size_t)nv * T);
  std::vector<u32> coin(T);
  for (u32 i = 0; i < nv; ++i) x[i] = mont_in(xp[i], m);
  for (u32 j = 0; j < T; ++j) xt[j] = mont_in(xtp[j], m);
  for (u32 e = 0; e < nv; ++e) {                       // shamir_prod_wide_kernel with t = nv - 1: every column is a basis column
    W4 lane[64];
    for (u32 l = 0; l < 64; ++l) {
      lane[l] = one(m);
      for (u32 i = l; i < nv; i += 64)
        if (i != e) lane[l] = mul(lane[l], sub(x[e], x[i], m), m);
    }
    u[e] = inv(meet_in_lane0(lane, m), m);
  }
  for (u32 j = 0; j < T; ++j) {                        // shamir_target_scale_wide_kernel
    W4 prod[64];
    u32 hit[64];
    for (u32 l = 0; l < 64; ++l) {
      prod[l] = one(m);
      hit[l] = NO_COLUMN;
      for (u32 i = l; i < nv; i += 64) {
        const W4 d = sub(xt[j], x[i], m);
        if (is0(d)) hit[l] = i;
        else prod[l] = mul(prod[l], d, m);
      }
    }
    for (u32 off = 32; off; off >>= 1) {
      W4 np[64];
      u32 nh[64];
      for (u32 l = 0; l < 64; ++l) {
        np[l] = mul(prod[l], prod[l ^ off], m);
        nh[l] = hit[l ^ off] < hit[l] ? hit[l ^ off] : hit[l];
      }
      memcpy(prod, np, sizeof prod);
      memcpy(hit, nh, sizeof hit);
    }
    scale[j] = prod[0];
    coin[j] = hit[0];
  }
  const W4 zero = {{0, 0, 0, 0}};
  for (u32 i0 = 0; i0 < nv; i0 += BATCH)               // shamir_cauchy_wide_kernel
    for (u32 j = 0; j < T; ++j) {
      const u32 cnt = nv - i0 < BATCH ? nv - i0 : BATCH;
      W4 run = one(m);
      for (u32 k = 0; k < cnt; ++k) {
        const W4 d = sub(xt[j], x[i0 + k], m);
        if (!is0(d)) run = mul(run, d, m);
        C[(size_t)(i0 + k) * T + j] = run;
      }
      W4 iv = inv(run, m);
      for (u32 k = cnt; k-- > 0;) {
        const W4 d = sub(xt[j], x[i0 + k], m);
        W4 v = zero;
        if (!is0(d)) {
          const W4 pre = k ? C[(size_t)(i0 + k - 1) * T + j] : one(m);
          v = mul(iv, pre, m);
          iv = mul(iv, d, m);
          v = mul(v, u[i0 + k], m);
        }
        C[(size_t)(i0 + k) * T + j] = v;
      }
    }
  const size_t ld = (size_t)D * NL;
  std::vector<i64> w((size_t)T * V * ld, 0);           // zeroed first: masked holders read 0
  for (size_t e = 0; e < (size_t)nv * T; ++e) {        // shamir_handover_digits_wide_kernel, thread e
    const u32 i = (u32)(e % nv), j = (u32)(e / nv);
    W4 mu = zero;
    if (coin[j] != NO_COLUMN) {
      if (coin[j] == i) mu = one(m);
    } else {
      mu = mul(scale[j], C[(size_t)i * T + j], m);
    }
    W4 tw = {{(u64)1 << limb_bits, 0, 0, 0}};
    tw = mont_in(tw, m);
    i64* out = w.data() + (size_t)j * V * ld + (size_t)col[i] * NL;
    for (u32 l = 0; l < NL; ++l) {
      W4 pl;
      wide_mont_out(mu.v, m, pl.v);
      wide_signed_digits(pl.v, m.p, b, V, out + l, ld);
      mu = mul(mu, tw, m);
    }
  }
  return w;
}

// shamir_wide_from_digits_kernel, thread i
static W4 kernel_fold(const u64* wide, const u32* status, size_t i, u32 V, u32 ww, u32 b, u32* status_out, const WideMod& m, const WideMont& mm) {
  const u64 zero[4] = {0, 0, 0, 0};
  u64 acc[4] = {0, 0, 0, 0};
  u32 st = 0;
  for (u32 v = V; v-- > 0;) {
    const u64* src = wide + (i * V + v) * ww;
    const u64 mag[4] = {src[0], ww > 1 ? src[1] : 0, ww > 2 ? src[2] : 0, ww > 3 ? src[3] : 0};
    const u32 sv = status[i * V + v];
    st |= sv;
    u64 r[4];
    wide_reduce_p(mag, mm, r);
    if ((sv & DEC_NEGATIVE) && (r[0] | r[1] | r[2] | r[3])) {
      u64 br = 0;
      for (int k = 0; k < 4; ++k) {
        const u64 s1 = mm.p[k] - r[k], s2 = s1 - br;
        br = (mm.p[k] < r[k]) | (s1 < br);
        r[k] = s2;
      }
    }
    wide_shl(r, m.shift);
    u32 rem = b;
    for (; rem > 31; rem -= 31) wide_step(acc, 1u << 31, zero, m);
    wide_step(acc, 1u << rem, r, m);
  }
  wide_shr(acc, m.shift);
  *status_out = st & ~DEC_NEGATIVE;
  W4 o;
  memcpy(o.v, acc, 32);
  return o;
}

static void print_w4(const W4& a) { printf(" %016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64, a.v[3], a.v[2], a.v[1], a.v[0]); }

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <prime in hex>...\n", argv[0]);
    return 2;
  }
  const u32 widths[4] = {8, 33, 60, 64};
  // holders 0, 2, 3, 5, 9 with holder 2 (the second of the list) masked out, or the list of "holders=i,j,.." (two at least, for
  // a prime whose field has no point 10); targets 0, the point of the third holder (valid; of the last one where there are
  // two), the point of the masked one
  std::vector<u64> idx = {0, 2, 3, 5, 9};
  int first = 1;
  if (strncmp(argv[1], "holders=", 8) == 0) {
    idx.clear();
    for (const char* s = argv[1] + 8; *s;) {
      char* end;
      idx.push_back(strtoull(s, &end, 10));
      if (end == s) return 2;
      s = *end == ',' ? end + 1 : end;
    }
    if (idx.size() < 2) return 2;
    first = 2;
  }
  for (int a = first; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p)) return 2;
    const WideMont mm = make_wide_mont(p);
    const WideMod m = make_wide_mod(p);
    rng_state = 0x5EED0000u + (u64)(a - first + 1);
    const u32 D = (u32)idx.size(), limb_bits = 52, NL = (m.bits + limb_bits - 1) / limb_bits;
    std::vector<W4> xp, xt = {W4{{0, 0, 0, 0}}, W4{{idx[D > 2 ? 2 : D - 1] + 1, 0, 0, 0}}, W4{{idx[1] + 1, 0, 0, 0}}};
    std::vector<u32> col;
    for (u32 d = 0; d < D; ++d)
      if (d != 1) {
        xp.push_back(W4{{idx[d] + 1, 0, 0, 0}});
        col.push_back(d);
      }
    for (u32 wi = 0; wi < 4; ++wi) {
      const u32 b = widths[wi], V = wide_signed_digit_count(m.bits, b);
      const std::vector<i64> w = kernel_weights(xp, col, xt, D, NL, V, limb_bits, b, mm);
      printf("W %d %u", a - first, b);
      for (i64 v : w) printf(" %" PRId64, v);
      printf("\n");
      // shamir_signed_digits_wide_kernel on eight words of any size
      printf("S %d %u", a - first, b);
      std::vector<i64> dg(V);
      for (u32 i = 0; i < 8; ++i) {
        const u64 val[4] = {rnd64(), rnd64(), rnd64(), i < 4 ? rnd64() : 0};
        u64 r[4];
        wide_reduce_p(val, mm, r);
        wide_signed_digits(r, mm.p, b, V, dg.data(), 1);
        for (i64 v : dg) printf(" %" PRId64, v);
      }
      printf("\n");
      // shamir_wide_from_digits_kernel on eight elements of V digits and ww = 1 + wi words
      const u32 ww = 1 + wi;
      std::vector<u64> wide((size_t)8 * V * ww);
      std::vector<u32> st((size_t)8 * V);
      for (u64& v : wide) v = rnd64();
      for (u32& v : st) v = (u32)(rnd64() & 7);
      printf("F %d %u", a - first, b);
      for (u32 i = 0; i < 8; ++i) {
        u32 so = 0;
        print_w4(kernel_fold(wide.data(), st.data(), i, V, ww, b, &so, m, mm));
        printf(" %u", so);
      }
      printf("\n");
    }
  }
  printf("SHAMIR_WIDE_HANDOVER_OK\n");
  return 0;
}

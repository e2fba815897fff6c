// The general product of the wide Shamir family (pvw_rs_amd/csrc/pvw_wide.h: wide_mul, Montgomery's product over 32-bit digits)
// and what is built on it -- the unreduced accumulator, the reduction of any four words, addition, subtraction and Fermat's
// inversion -- against a schoolbook product and long division in base 2^64 with unsigned __int128 intermediates (Knuth's
// algorithm D).  Stand-alone: shamir_wide_mul <cases> <prime in hex>...
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pvw_wide.h"

using namespace pvw;

static u64 rng_state;
static u64 rnd64() {   // splitmix64
  u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// rem[0..n) = u[0..ulen) mod v[0..n); v[n - 1] != 0, ulen >= n
static void divrem(const u64* u, int ulen, const u64* v, int n, u64* rem) {
  if (n == 1) {
    u128 r = 0;
    for (int i = ulen - 1; i >= 0; --i) r = ((r << 64) | u[i]) % v[0];
    rem[0] = (u64)r;
    return;
  }
  const int s = __builtin_clzll(v[n - 1]);
  u64 vn[8], un[16];
  for (int i = n - 1; i > 0; --i) vn[i] = s ? (v[i] << s) | (v[i - 1] >> (64 - s)) : v[i];
  vn[0] = v[0] << s;
  un[ulen] = s ? u[ulen - 1] >> (64 - s) : 0;
  for (int i = ulen - 1; i > 0; --i) un[i] = s ? (u[i] << s) | (u[i - 1] >> (64 - s)) : u[i];
  un[0] = u[0] << s;
  for (int j = ulen - n; j >= 0; --j) {
    const u128 num = ((u128)un[j + n] << 64) | un[j + n - 1];
    u128 qhat = num / vn[n - 1], rhat = num % vn[n - 1];
    while ((qhat >> 64) || qhat * vn[n - 2] > ((rhat << 64) | un[j + n - 2])) {
      --qhat;
      rhat += vn[n - 1];
      if (rhat >> 64) break;
    }
    u128 carry = 0;
    u64 borrow = 0;
    for (int i = 0; i < n; ++i) {
      const u128 p = (u128)(u64)qhat * vn[i] + carry;
      carry = p >> 64;
      const u64 sub = (u64)p, a = un[i + j], d1 = a - sub, d2 = d1 - borrow;
      borrow = (a < sub) | (d1 < borrow);
      un[i + j] = d2;
    }
    {
      const u64 a = un[j + n], sub = (u64)carry, d1 = a - sub, d2 = d1 - borrow;
      borrow = (a < sub) | (d1 < borrow);
      un[j + n] = d2;
    }
    if (borrow) {   // qhat was one too large: add back
      u64 c = 0;
      for (int i = 0; i < n; ++i) {
        const u128 t = (u128)un[i + j] + vn[i] + c;
        un[i + j] = (u64)t;
        c = (u64)(t >> 64);
      }
      un[j + n] += c;
    }
  }
  for (int i = 0; i < n; ++i) rem[i] = s ? (un[i] >> s) | (un[i + 1] << (64 - s)) : un[i];
}

// out[0..9) += a b: schoolbook in base 2^64
static void mul_add(const u64* a, const u64* b, u64* out) {
  u64 prod[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    u64 c = 0;
    for (int j = 0; j < 4; ++j) {
      const u128 t = (u128)a[i] * b[j] + prod[i + j] + c;
      prod[i + j] = (u64)t;
      c = (u64)(t >> 64);
    }
    prod[i + 4] = c;
  }
  u64 c = 0;
  for (int i = 0; i < 9; ++i) {
    const u128 t = (u128)out[i] + (i < 8 ? prod[i] : 0) + c;
    out[i] = (u64)t;
    c = (u64)(t >> 64);
  }
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

static void random_below(const u64 (&p)[4], const WideMod& m, u64 (&out)[4]) {
  for (;;) {
    for (int i = 0; i < 4; ++i) out[i] = rnd64();
    wide_shl(out, m.shift);
    wide_shr(out, m.shift);
    if (wide_less(out, p)) return;
  }
}

static int fail(const char* what, const char* prime, long i) {
  printf("%s MISMATCH prime %s case %ld\n", what, prime, i);
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long cases = atol(argv[1]);
  for (int a = 2; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p) || !(p[0] & 1)) return 2;
    const WideMod sm = make_wide_mod(p);
    const WideMont m = make_wide_mont(p);
    int n = 4;
    while (n > 1 && !p[n - 1]) --n;
    const u64 pm1[4] = {p[0] - 1, p[1], p[2], p[3]};
    // the constants: one = 2^256 mod p, r2 = 2^512 mod p, n0 p = -1 mod 2^32
    {
      u64 pw[9] = {0, 0, 0, 0, 1, 0, 0, 0, 0}, want[4] = {0, 0, 0, 0};
      divrem(pw, 5, p, n, want);
      if (memcmp(want, m.one, 32) != 0) return fail("ONE", argv[a], 0);
      pw[4] = 0;
      pw[8] = 1;
      memset(want, 0, 32);
      divrem(pw, 9, p, n, want);
      if (memcmp(want, m.r2, 32) != 0) return fail("R2", argv[a], 0);
      if ((u32)(m.n0 * (u32)p[0]) != 0xFFFFFFFFu) return fail("N0", argv[a], 0);
    }
    rng_state = 0xC0FFEE00 + (u64)a;
    u64 sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // the running sum of the products, exact
    u32 T[16];                                   // the same sum in the kernel's accumulator, with b in Montgomery form
    wide_acc_zero(T);
    for (long i = 0; i < cases; ++i) {
      // operands 0, 1, p - 1, random in every combination first (the pair (p - 1, p - 1) among them), then random ones
      const bool edge = i < 16 * 8;
      const int ak = edge ? (int)(i % 4) : 3, bk = edge ? (int)((i / 4) % 4) : 3;
      u64 x[4], y[4];
      auto pick = [&](int k, u64 (&o)[4]) {
        memset(o, 0, 32);
        if (k == 1) o[0] = 1;
        else if (k == 2) memcpy(o, pm1, 32);
        else if (k == 3) random_below(p, sm, o);
      };
      pick(ak, x);
      pick(bk, y);
      u64 prod[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, want[4] = {0, 0, 0, 0}, got[4];
      mul_add(x, y, prod);
      divrem(prod, 8, p, n, want);
      wide_mul(x, y, m, got);
      if (memcmp(got, want, 32) != 0) return fail("MUL", argv[a], i);
      // the accumulator: T += x (y R), reduced every 61 terms and at the end; the exact sum restarts with it
      u64 ym[4];
      u32 P[16];
      wide_mont_in(y, m, ym);
      wide_mul_full(x, ym, P);
      wide_acc_add(T, P, m);
      mul_add(x, y, sum);
      if (i % 61 == 60 || i == cases - 1) {
        u64 ws[4] = {0, 0, 0, 0}, gs[4];
        divrem(sum, 9, p, n, ws);
        wide_redc(T, m, gs);
        if (memcmp(gs, ws, 32) != 0) return fail("ACC", argv[a], i);
        memset(sum, 0, sizeof sum);
        wide_acc_zero(T);
      }
      if (i % 16 == 0) {   // any four words, read mod p
        u64 w[4], r[4], wr[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) w[k] = i % 64 == 0 ? ~(u64)0 : rnd64();
        divrem(w, 4, p, n, wr);
        wide_reduce_p(w, m, r);
        if (memcmp(r, wr, 32) != 0) return fail("REDUCE", argv[a], i);
        // any words times an element below p
        memset(prod, 0, sizeof prod);
        memset(want, 0, 32);
        mul_add(w, y, prod);
        divrem(prod, 8, p, n, want);
        wide_mul(w, y, m, got);
        if (memcmp(got, want, 32) != 0) return fail("MUL ANY", argv[a], i);
      }
      {   // x + y and x - y mod p
        u64 s5[5], wsum[4] = {0, 0, 0, 0}, gsum[4], gdiff[4];
        u128 c = 0;
        for (int k = 0; k < 4; ++k) {
          c += (u128)x[k] + y[k];
          s5[k] = (u64)c;
          c >>= 64;
        }
        s5[4] = (u64)c;
        divrem(s5, 5, p, n, wsum);
        memcpy(gsum, x, 32);
        wide_add_p(gsum, y, m);
        if (memcmp(gsum, wsum, 32) != 0) return fail("ADD", argv[a], i);
        memcpy(gdiff, wsum, 32);
        wide_sub_p(gdiff, y, m);                 // (x + y) - y = x
        if (memcmp(gdiff, x, 32) != 0) return fail("SUB", argv[a], i);
      }
      if (i % 1024 == 3 && (x[0] | x[1] | x[2] | x[3])) {   // Fermat: x^-1 x = 1
        u64 xm[4], inv[4], one[4];
        wide_mont_in(x, m, xm);
        wide_mont_inv(xm, m, inv);
        wide_mont_mul(inv, x, m, one);           // (x^-1 R) x R^-1 = 1
        const u64 w1[4] = {1, 0, 0, 0};
        if (memcmp(one, w1, 32) != 0) return fail("INV", argv[a], i);
      }
    }
  }
  printf("SHAMIR_WIDE_MUL_OK\n");
  return 0;
}

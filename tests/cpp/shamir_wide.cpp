// The Horner step of the wide Shamir kernel (pvw_rs_amd/csrc/pvw_wide.h: acc <- (acc x + add) mod p by a quotient estimate
// and one correction) and the word reduction built on it, against schoolbook long division in base 2^64 with unsigned
// __int128 intermediates (Knuth's algorithm D).  Stand-alone: shamir_wide <cases> <prime in hex>...
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
    // multiply and subtract
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

static bool parse_hex(const char* h, u64 (&out)[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (h[0] == '0' && (h[1] == 'x' || h[1] == 'X')) h += 2;
  const size_t len = strlen(h);
  if (len == 0 || len > 64) return false;
  for (size_t i = 0; i < len; ++i) {
    const char ch = h[len - 1 - i];
    u64 dgt;
    if (ch >= '0' && ch <= '9') dgt = (u64)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') dgt = (u64)(ch - 'a' + 10);
    else if (ch >= 'A' && ch <= 'F') dgt = (u64)(ch - 'A' + 10);
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

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long cases = atol(argv[1]);
  for (int a = 2; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p) || !(p[0] & 1)) return 2;
    const WideMod m = make_wide_mod(p);
    int n = 4;
    while (n > 1 && !p[n - 1]) --n;
    u64 pm1[4] = {p[0] - 1, p[1], p[2], p[3]};
    rng_state = 0x5EED0000 + (u64)a;
    for (long i = 0; i < cases; ++i) {
      // the edge combinations first, then random operands
      const bool edge = i < 45 * 20;
      const int xk = edge ? (int)(i % 5) : 4, ak = edge ? (int)((i / 5) % 3) : 2, bk = edge ? (int)((i / 15) % 3) : 2;
      const u32 xs[4] = {1u, 2u, 1u << 16, 0xFFFFFFFFu};
      const u32 x = xk < 4 ? xs[xk] : (u32)(rnd64() >> (32 + (rnd64() % 32)));
      u64 acc[4], add[4];
      if (ak == 0) memset(acc, 0, 32); else if (ak == 1) memcpy(acc, pm1, 32); else random_below(p, m, acc);
      if (bk == 0) memset(add, 0, 32); else if (bk == 1) memcpy(add, pm1, 32); else random_below(p, m, add);
      // T = acc x + add, five words
      u64 T[5];
      u128 c = 0;
      for (int k = 0; k < 4; ++k) {
        c += (u128)acc[k] * x + add[k];
        T[k] = (u64)c;
        c >>= 64;
      }
      T[4] = (u64)c;
      u64 want[4] = {0, 0, 0, 0};
      divrem(T, 5, p, n, want);
      u64 got[4], sadd[4];
      memcpy(got, acc, 32);
      memcpy(sadd, add, 32);
      wide_shl(got, m.shift);
      wide_shl(sadd, m.shift);
      wide_step(got, x, sadd, m);
      wide_shr(got, m.shift);
      if (memcmp(got, want, 32) != 0) {
        printf("STEP MISMATCH prime %s case %ld x %u\n", argv[a], i, x);
        return 1;
      }
      if (i % 16 == 0) {   // any four words, reduced by the same step
        u64 w[4], r[4], wr[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) w[k] = i % 64 == 0 ? ~(u64)0 : rnd64();
        divrem(w, 4, p, n, wr);
        wide_reduce_scaled(w, m, r);
        wide_shr(r, m.shift);
        if (memcmp(r, wr, 32) != 0) {
          printf("REDUCE MISMATCH prime %s case %ld\n", argv[a], i);
          return 1;
        }
      }
    }
  }
  printf("SHAMIR_WIDE_OK\n");
  return 0;
}

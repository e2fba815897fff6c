// pvw_wide.h -- arithmetic in Z_p for an odd prime p < 2^256, shared by host and gfx950 device code.
// Two parts: the Horner step of the dealing end, on scaled elements (here), and the general product of the receiving end,
// Montgomery's on plain elements (further down, with its own argument).
//
// A wide element is four little-endian u64 words.  The first part works on SCALED elements: v' = v * 2^s with
// s = 256 - bitlen(p), modulo pn = p * 2^s, whose bit 255 is set.  Addition and multiplication by an integer commute with the
// scaling, (acc' x + add') mod pn = ((acc x + add) mod p) * 2^s, so a whole Horner walk runs scaled: its inputs are shifted left
// once and its result is shifted right once, and the quotient estimate below always finds the modulus in the same place.
//
// Its one arithmetic routine is wide_step: acc <- (acc x + add) mod pn for acc, add < pn and x < 2^32.  With the shares'
// points x = i + 1 <= n < 2^32 Horner from the top coefficient needs nothing else: 8 multiply-adds (v_mad_u64_u32) for
// T = acc x + add < pn 2^32, one quotient below 2^32, 8 more for T - q pn, one conditional subtraction.
//
// Quotient.  q = floor(T / pn) < 2^32.  Let a = floor(T / 2^224) < 2^64 (T < 2^288), d = floor(pn / 2^192) + 1 in (2^63, 2^64],
// rec = floor(2^127 / d) < 2^64 and qe = floor(a rec / 2^95) = mulhi64(a, rec) >> 31.
//   qe <= q:  a rec / 2^95 <= a 2^32 / d <= T / (2^192 d) < T / pn, because 2^192 d > pn.
//   qe >= q - 1:  a > T / 2^224 - 1 and rec > 2^127 / d - 1 give a rec / 2^95 > T / (2^192 d) - T / 2^319 - 2^32 / d
//   > T / (2^192 d) - 2^-30 (T < 2^288, d > 2^63); and T / pn - T / (2^192 d) = T (2^192 d - pn) / (pn 2^192 d) <= (T / pn) / d
//   < 2^32 / 2^63 = 2^-31.  So a rec / 2^95 > T / pn - 2^-29 >= q - 2^-29 and its floor is at least q - 1.
// Hence T - qe pn lies in [0, 2 pn) < 2^257 and ONE conditional subtraction of pn ends the step.
//
// Words that are not known to be below p (secrets, explicit coefficients, limb sums) are reduced by the same step: Horner
// over the word's digits from the top with x = 2^dw.  A digit must be below p to be an addend, so dw = min(16, bitlen(p) - 1):
// 16 digits of 16 bits for every p >= 2^16, narrower digits below that.
#pragma once
#include "pvw_arith.h"
#include "pvw_chacha.h"

namespace pvw {

struct WideMod {
  u64 pn[4];    // p << shift: bit 255 set
  u64 rec;      // floor(2^127 / (pn[3] + 1))
  u32 shift;    // 256 - bits
  u32 bits;     // bitlen(p) >= 2
};

PVW_HD bool wide_less(const u64 (&a)[4], const u64 (&b)[4]) {
  bool lt = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) lt = a[i] < b[i] || (a[i] == b[i] && lt);
  return lt;
}

// a <<= s (mod 2^256) and a >>= s for s < 256, without runtime-indexed registers: whole words in two stages, then bits
PVW_HD void wide_shl(u64 (&a)[4], u32 s) {
  if (s & 128) { a[3] = a[1]; a[2] = a[0]; a[1] = 0; a[0] = 0; }
  if (s & 64) { a[3] = a[2]; a[2] = a[1]; a[1] = a[0]; a[0] = 0; }
  const u32 b = s & 63;
  if (b) {
    a[3] = (a[3] << b) | (a[2] >> (64 - b));
    a[2] = (a[2] << b) | (a[1] >> (64 - b));
    a[1] = (a[1] << b) | (a[0] >> (64 - b));
    a[0] <<= b;
  }
}
PVW_HD void wide_shr(u64 (&a)[4], u32 s) {
  if (s & 128) { a[0] = a[2]; a[1] = a[3]; a[2] = 0; a[3] = 0; }
  if (s & 64) { a[0] = a[1]; a[1] = a[2]; a[2] = a[3]; a[3] = 0; }
  const u32 b = s & 63;
  if (b) {
    a[0] = (a[0] >> b) | (a[1] << (64 - b));
    a[1] = (a[1] >> b) | (a[2] << (64 - b));
    a[2] = (a[2] >> b) | (a[3] << (64 - b));
    a[3] >>= b;
  }
}

// acc <- (acc x + add) mod pn; acc, add < pn, x < 2^32 (the proof of the single correction is at the top of the file)
PVW_HD void wide_step(u64 (&acc)[4], u32 x, const u64 (&add)[4], const WideMod& m) {
  u32 T[9];
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 ai = (u32)(acc[i >> 1] >> (32 * (i & 1))), di = (u32)(add[i >> 1] >> (32 * (i & 1)));
    const u64 v = (u64)ai * x + di + c;          // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
    T[i] = (u32)v;
    c = v >> 32;
  }
  T[8] = (u32)c;
  const u64 a = ((u64)T[8] << 32) | T[7];
  const u32 q = (u32)(mulhi64(a, m.rec) >> 31);  // q or q - 1 of floor(T / pn) < 2^32
  // r = T - q pn, below 2 pn: 257 bits
  u32 r[9];
  u64 mc = 0;
  i64 bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 pi = (u32)(m.pn[i >> 1] >> (32 * (i & 1)));
    const u64 v = (u64)pi * q + mc;
    mc = v >> 32;
    const i64 dlt = (i64)T[i] - (i64)(u32)v + bw;   // in (-2^32, 2^32)
    r[i] = (u32)dlt;
    bw = dlt >> 32;                                 // 0 or -1
  }
  const u32 top = (u32)((i64)T[8] - (i64)mc + bw);  // 0 or 1
  u64 w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (u64)r[2 * i] | ((u64)r[2 * i + 1] << 32);
  if (top || !wide_less(w, m.pn)) {
    u64 br = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u64 s1 = w[i] - m.pn[i], s2 = s1 - br;
      br = (w[i] < m.pn[i]) | (s1 < br);
      w[i] = s2;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = w[i];
}

// digit width of the reduction below
PVW_HD u32 wide_digit_bits(const WideMod& m) { return m.bits - 1 < 16 ? m.bits - 1 : 16; }

// out = (w mod p) scaled, for any four words at w (memory: the digits are fetched by a runtime index)
PVW_HD void wide_reduce_scaled(const u64* w, const WideMod& m, u64 (&out)[4]) {
  const u32 dw = wide_digit_bits(m), nd = (256 + dw - 1) / dw;
  const u64 mask = ((u64)1 << dw) - 1;
  u64 acc[4] = {0, 0, 0, 0};
  for (u32 k = nd; k-- > 0;) {
    const u32 pos = k * dw, wi = pos >> 6, off = pos & 63;
    u64 dg = w[wi] >> off;
    if (off + dw > 64 && wi < 3) dg |= w[wi + 1] << (64 - off);
    u64 add[4] = {dg & mask, 0, 0, 0};
    wide_shl(add, m.shift);                        // digit < 2^(bits - 1) <= p: the addend is below pn
    wide_step(acc, (u32)1 << dw, add, m);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = acc[i];
}

// the same for one word v (the upper words' digits are 0 and leave acc = 0): the digits come out of a register by shifts
PVW_HD void wide_reduce_word_scaled(u64 v, const WideMod& m, u64 (&out)[4]) {
  const u32 dw = wide_digit_bits(m), nd = (64 + dw - 1) / dw;
  const u64 mask = ((u64)1 << dw) - 1;
  u64 acc[4] = {0, 0, 0, 0};
  for (u32 k = nd; k-- > 0;) {
    u64 add[4] = {(v >> (k * dw)) & mask, 0, 0, 0};
    wide_shl(add, m.shift);
    wide_step(acc, (u32)1 << dw, add, m);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = acc[i];
}

// a_{d,j} scaled: the first accepted draw of the stream (key, (DOM_SHAMIR << 32) | j).  An attempt is four consecutive
// next_u64() words, word 0 least significant, masked to the low bitlen(p) bits and accepted when below p.  Shifting the 256-bit
// draw left by `shift` drops exactly the bits the mask drops, so the scaled candidate is the shifted draw and the test is
// against pn.  A block holds two attempts, tried in order with static word indices.
PVW_HD void wide_draw_scaled(const ChaChaKey& key, u32 domain, u32 j, const WideMod& m, u64 (&out)[4]) {
  ChaChaRng g;
  g.init(key, domain, j);
  for (;;) {
    g.refill();
    bool got = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u64 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (u64)g.buf[8 * h + 2 * i] | ((u64)g.buf[8 * h + 2 * i + 1] << 32);
      wide_shl(v, m.shift);
      if (!got && wide_less(v, m.pn)) {
        got = true;
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = v[i];
      }
    }
    if (got) return;
  }
}

// ------------------------------------------------------------------------ the general product
// wide_step multiplies by x < 2^32 only.  Checked reconstruction multiplies two field elements: a share by a Lagrange weight.
// The product is Montgomery's over eight 32-bit digits, R = 2^256, on PLAIN elements (no scaling), because of who pays for
// the conversions: the weights are public and made once, so they are stored as W R mod p; the shares are secret, arrive as
// they are and need no conversion at all, for REDC(share * (W R)) = share W mod p is a plain field element.
//
// Three pieces, all with static digit indices only (every loop below is fully unrolled):
//   wide_mul_full   P = a b, sixteen digits, schoolbook by rows: 64 multiply-adds (v_mad_u64_u32).  In row i the running value
//                   a_i b_j + P[i+j] + c <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1 fits a u64.
//   wide_acc_add    T <- T + P, kept BELOW p R.  Invariant T < p R.  One operand of P is below p and the other below R, so
//                   P <= (p - 1)(R - 1) < p R and T + P < 2 p R < 2^513: sixteen digits and one carry bit.  T + P >= p R holds
//                   exactly when the carry is set or the upper eight digits are >= p (the lower eight are below R), and then
//                   p is taken off the upper half ONCE: T + P - p R < p R again.  A sum of any number of products is therefore
//                   accumulated unreduced at 64 multiply-adds a term, and reduced once at the end.
//   wide_redc       out = T R^-1 mod p for T < p R.  Row i takes m = T[i] n0 mod 2^32 (n0 = -p^-1 mod 2^32) and adds m p 2^(32 i),
//                   which clears digit i; after eight rows the lower half is 0 and the upper half plus the last carry is
//                   U = (T + M p) / R with M < R, so U < (p R + R p) / R = 2 p and U = T R^-1 (mod p): ONE conditional
//                   subtraction of p ends it (taken when the carry is set or the eight digits are >= p).  Carries: row i's
//                   last carry c and the bit e left by row i - 1 go into digit i + 8 as T[i+8] + c + e <= 2 (2^32 - 1) + 1;
//                   digit i + 8 is touched by later rows only after that, and digit i + 9 by nobody before row i + 1 ends.
// wide_mont_mul(a, b) = REDC(a b) = a b R^-1 mod p, below p, for a < R and b < p (or the other way round).
// wide_mul(a, b) = REDC(REDC(a b) r2) with r2 = R^2 mod p: a b mod p for a < R, b < p -- the general product in Z_p.
// Any four words w are read mod p by the same two steps: wide_mont_in(w) = REDC(w r2) = w R mod p (w < R, r2 < p) and
// wide_redc of that alone (upper half 0: T < R <= p R) gives w mod p.
// Inversion is Fermat's, a^(p-2), 256 squarings and a product per set bit: about 380 products for a 256-bit p.
struct WideMont {
  u64 p[4];     // the modulus: odd, >= 3
  u64 r2[4];    // 2^512 mod p
  u64 one[4];   // 2^256 mod p: 1 in Montgomery form
  u32 n0;       // -p^-1 mod 2^32
};

#define PVW_WIDE_DIGIT(a, i) ((u32)((a)[(i) >> 1] >> (32 * ((i) & 1))))

PVW_HD void wide_mul_full(const u64 (&a)[4], const u64 (&b)[4], u32 (&P)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) P[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 ai = PVW_WIDE_DIGIT(a, i);
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const u64 v = (u64)ai * PVW_WIDE_DIGIT(b, j) + P[i + j] + c;
      P[i + j] = (u32)v;
      c = v >> 32;
    }
    P[i + 8] = (u32)c;
  }
}

// h (eight digits, with `top` as the ninth) >= p ? h - p : h, mod 2^256
PVW_HD void wide_cond_sub(u32 (&h)[8], u32 top, const u64 (&p)[4]) {
  bool lt = false;                                   // h < p over the eight digits
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 pi = PVW_WIDE_DIGIT(p, i);
    lt = h[i] < pi || (h[i] == pi && lt);
  }
  if (top || !lt) {
    i64 bw = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const i64 d = (i64)h[i] - (i64)PVW_WIDE_DIGIT(p, i) + bw;   // in (-2^32, 2^32)
      h[i] = (u32)d;
      bw = d >> 32;                                  // 0 or -1
    }
  }
}

PVW_HD void wide_acc_zero(u32 (&T)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) T[i] = 0;
}

// T <- T + P - (T + P >= p R ? p R : 0); T < p R, P < p R
PVW_HD void wide_acc_add(u32 (&T)[16], const u32 (&P)[16], const WideMont& m) {
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const u64 v = (u64)T[i] + P[i] + c;
    T[i] = (u32)v;
    c = v >> 32;
  }
  u32 h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = T[8 + i];
  wide_cond_sub(h, (u32)c, m.p);
#pragma unroll
  for (int i = 0; i < 8; ++i) T[8 + i] = h[i];
}

// out = T R^-1 mod p, below p; T < p R (T is used up)
PVW_HD void wide_redc(u32 (&T)[16], const WideMont& m, u64 (&out)[4]) {
  u32 e = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 q = T[i] * m.n0;
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const u64 v = (u64)q * PVW_WIDE_DIGIT(m.p, j) + T[i + j] + c;
      T[i + j] = (u32)v;
      c = v >> 32;
    }
    const u64 s = (u64)T[i + 8] + c + e;
    T[i + 8] = (u32)s;
    e = (u32)(s >> 32);
  }
  u32 h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = T[8 + i];
  wide_cond_sub(h, e, m.p);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = (u64)h[2 * i] | ((u64)h[2 * i + 1] << 32);
}

// out = a b R^-1 mod p; a < 2^256 and b < p (or the other way round).  out may be a or b.
PVW_HD void wide_mont_mul(const u64 (&a)[4], const u64 (&b)[4], const WideMont& m, u64 (&out)[4]) {
  u32 T[16];
  wide_mul_full(a, b, T);
  wide_redc(T, m, out);
}
// out = a b mod p; a < 2^256, b < p
PVW_HD void wide_mul(const u64 (&a)[4], const u64 (&b)[4], const WideMont& m, u64 (&out)[4]) {
  u64 t[4];
  wide_mont_mul(a, b, m, t);
  wide_mont_mul(t, m.r2, m, out);
}
// out = w R mod p for any four words w, and back: out = a R^-1 mod p for a < 2^256
PVW_HD void wide_mont_in(const u64 (&w)[4], const WideMont& m, u64 (&out)[4]) { wide_mont_mul(w, m.r2, m, out); }
PVW_HD void wide_mont_out(const u64 (&a)[4], const WideMont& m, u64 (&out)[4]) {
  u32 T[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) { T[i] = PVW_WIDE_DIGIT(a, i); T[8 + i] = 0; }
  wide_redc(T, m, out);
}
// out = w mod p for any four words w
PVW_HD void wide_reduce_p(const u64 (&w)[4], const WideMont& m, u64 (&out)[4]) {
  u64 t[4];
  wide_mont_in(w, m, t);
  wide_mont_out(t, m, out);
}

// a <- (a + b) mod p and a <- (a - b) mod p for a, b < p
PVW_HD void wide_add_p(u64 (&a)[4], const u64 (&b)[4], const WideMont& m) {
  u32 h[8];
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u64 v = (u64)PVW_WIDE_DIGIT(a, i) + PVW_WIDE_DIGIT(b, i) + c;
    h[i] = (u32)v;
    c = v >> 32;
  }
  wide_cond_sub(h, (u32)c, m.p);                       // a + b < 2 p
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = (u64)h[2 * i] | ((u64)h[2 * i + 1] << 32);
}
PVW_HD void wide_sub_p(u64 (&a)[4], const u64 (&b)[4], const WideMont& m) {
  u64 r[4], br = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 s1 = a[i] - b[i], s2 = s1 - br;
    br = (a[i] < b[i]) | (s1 < br);
    r[i] = s2;
  }
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                        // + p where the difference went below 0
    const u64 add = br ? m.p[i] : 0, s1 = r[i] + add, s2 = s1 + c;
    c = (s1 < add) | (s2 < s1);
    a[i] = s2;
  }
}

// out = a^-1 in Montgomery form for a != 0 in Montgomery form: a^(p-2), bits from the top, the exponent's words by static index
PVW_HD void wide_mont_inv(const u64 (&a)[4], const WideMont& m, u64 (&out)[4]) {
  u64 e[4], br = 2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 v = m.p[i];
    e[i] = v - br;
    br = v < br;
  }
  u64 r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = m.one[i];
#pragma unroll
  for (int w = 3; w >= 0; --w) {
    u64 ew = e[w];
#pragma unroll 1
    for (int b = 0; b < 64; ++b) {
      wide_mont_mul(r, r, m, r);
      if (ew >> 63) wide_mont_mul(r, a, m, r);
      ew <<= 1;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = r[i];
}

// ------------------------------------------------------------------------ signed digits
// A value x below p is cut into V = ceil((bitlen(p) + 1) / b) signed digits of b bits, 8 <= b <= 64, B = 2^b: the centred residue
// xc in (-p/2, p/2] is xc = sum_v c_v B^v with every c_v in [-B/2, B/2).  Digits 0 .. V - 2 are xc mod B taken centred, xc <- (xc - c_v) / B;
// the top digit is what is left.  It fits: |xc| < 2^(bits - 1), a centred step takes |xc| to at most |xc| / B + 1/2, so after
// V - 1 steps |xc| < 2^(bits - 1 - b (V - 1)) + 1/2 + 1/(2 (B - 1)) <= 2^(b - 2) + 0.51 (b V >= bits + 1): the integer is at most
// 2^(b - 2).  (With V = ceil(bits / b) the same bound is 2^(b - 1) + 0.51 and the chain does not close: B = 4, V = 2, x = 6.)
// xc travels as 256 bits of two's complement (|xc| < 2^255): the centred low digit is the low b bits read as signed, and
// (xc - c) / B is the arithmetic shift plus the bit b - 1 of the low digit.  Static word indices only.
PVW_HD u32 wide_signed_digit_count(u32 bits, u32 b) { return (bits + 1 + b - 1) / b; }

// x <- the centred residue of x (below p) as two's complement over four words
PVW_HD void wide_centre(u64 (&x)[4], const u64 (&p)[4]) {
  u64 h[4] = {p[0], p[1], p[2], p[3]};
  wide_shr(h, 1);                                        // floor(p / 2): x > h means x - p is the centred residue
  if (!wide_less(h, x)) return;
  u64 br = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 s1 = x[i] - p[i], s2 = s1 - br;
    br = (x[i] < p[i]) | (s1 < br);
    x[i] = s2;
  }
}
// the next digit of x (two's complement, four words), x <- (x - digit) / 2^b; 1 <= b <= 64
PVW_HD i64 wide_signed_digit_next(u64 (&x)[4], u32 b) {
  const u64 low = b == 64 ? x[0] : x[0] & (((u64)1 << b) - 1);
  const u64 carry = (low >> (b - 1)) & 1;
  const i64 c = b == 64 ? (i64)low : (i64)(low - (carry << b));
  const u64 sign = (u64)((i64)x[3] >> 63);
  if (b == 64) {
    x[0] = x[1]; x[1] = x[2]; x[2] = x[3]; x[3] = sign;
  } else {
    x[0] = (x[0] >> b) | (x[1] << (64 - b));
    x[1] = (x[1] >> b) | (x[2] << (64 - b));
    x[2] = (x[2] >> b) | (x[3] << (64 - b));
    x[3] = (u64)((i64)x[3] >> b);
  }
  u64 cy = carry;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 s = x[i] + cy;
    cy = s < cy;
    x[i] = s;
  }
  return c;
}
// digits[v * stride] = c_v for v < V, of x below p
PVW_HD void wide_signed_digits(const u64 (&x)[4], const u64 (&p)[4], u32 b, u32 V, i64* digits, size_t stride) {
  u64 t[4] = {x[0], x[1], x[2], x[3]};
  wide_centre(t, p);
  for (u32 v = 0; v + 1 < V; ++v) digits[(size_t)v * stride] = wide_signed_digit_next(t, b);
  digits[(size_t)(V - 1) * stride] = (i64)t[0];
}

// host: the constants of p (odd, >= 3, below 2^256), for the product above and for the step at the top
inline WideMont make_wide_mont(const u64 p[4]) {
  WideMont m;
  for (int i = 0; i < 4; ++i) m.p[i] = p[i];
  u32 inv = (u32)p[0];                                 // p p = 1 mod 8; each Newton step doubles the correct bits
  for (int i = 0; i < 5; ++i) inv *= 2 - (u32)p[0] * inv;
  m.n0 = 0u - inv;
  u64 v[4] = {1, 0, 0, 0};                             // 2^k mod p by doubling: v < p, 2 v < 2^257
  for (int k = 0; k < 512; ++k) {
    const u64 top = v[3] >> 63;
    wide_shl(v, 1);
    if (top || !wide_less(v, m.p)) {
      u64 br = 0;
      for (int i = 0; i < 4; ++i) {
        const u64 s1 = v[i] - m.p[i], s2 = s1 - br;
        br = (v[i] < m.p[i]) | (s1 < br);
        v[i] = s2;
      }
    }
    if (k == 255) for (int i = 0; i < 4; ++i) m.one[i] = v[i];
  }
  for (int i = 0; i < 4; ++i) m.r2[i] = v[i];
  return m;
}

inline WideMod make_wide_mod(const u64 p[4]) {
  WideMod m;
  u32 bits = 0;
  for (int i = 3; i >= 0 && !bits; --i)
    if (p[i]) bits = 64 * (u32)i + 64 - (u32)__builtin_clzll(p[i]);
  m.bits = bits;
  m.shift = 256 - bits;
  u64 t[4] = {p[0], p[1], p[2], p[3]};
  wide_shl(t, m.shift);
  for (int i = 0; i < 4; ++i) m.pn[i] = t[i];
  const u64 d = m.pn[3] + 1;
  m.rec = d ? (u64)(((u128)1 << 127) / d) : (u64)1 << 63;
  return m;
}

}  // namespace pvw

// pvw_wide.h -- arithmetic in Z_p for an odd prime p < 2^256, shared by host and gfx950 device code.
//
// A wide element is four little-endian u64 words.  Everything below works on SCALED elements: v' = v * 2^s with
// s = 256 - bitlen(p), modulo pn = p * 2^s, whose bit 255 is set.  Addition and multiplication by an integer commute with the
// scaling, (acc' x + add') mod pn = ((acc x + add) mod p) * 2^s, so a whole Horner walk runs scaled: its inputs are shifted left
// once and its result is shifted right once, and the quotient estimate below always finds the modulus in the same place.
//
// The one arithmetic routine is wide_step: acc <- (acc x + add) mod pn for acc, add < pn and x < 2^32.  With the shares'
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

// host: the constants of p (odd, >= 3, below 2^256)
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

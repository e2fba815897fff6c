// Host check of pvw_rs_amd/csrc/pvw_arith.h (the arithmetic every kernel is built from) against unsigned __int128 `%`,
// for the moduli given on stdin (decimal, whitespace-separated): reduce128, mulmod, mulmod_shoup, signed_residue, the lazy
// accumulator up to its 2^32-term bound, the l-point NTT against direct evaluation, and the digit step of the GEMM operands
// (mul256_consts + mulmod_shoup), and reduce_word on unreduced caller words: alone, ahead of the l-point NTTs and ahead
// of the balanced digits of the GEMM operands.  Prints one "FAIL <what> q=<q> ..." line per failing (check, modulus) and ends with
// "ARITH_EDGES_OK <moduli>" when nothing failed.
//
// -DPVW_PARENT_DIGIT_STEP: the digit step through the constant pair the kernels used before mul256_consts (w = 256,
// wp = floor(2^128 / q) >> 56), which the test suite expects to fail exactly for q < 256.
// -DPVW_RAW_WORDS: the unreduced words go into the NTTs and the digits without reduce_word, as the kernels took them
// before it; the test suite expects the raw_words checks to fail then.
#include <cinttypes>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "pvw_arith.h"

using namespace pvw;

static std::set<std::string> g_failed;   // "what q" pairs already reported
static int g_fail = 0;

static bool check(bool ok, const char* what, u64 q, u64 a = 0, u64 b = 0) {
  if (ok) return true;
  ++g_fail;
  std::string key = std::string(what) + " " + std::to_string(q);
  if (g_failed.insert(key).second) printf("FAIL %s q=%" PRIu64 " a=%#" PRIx64 " b=%#" PRIx64 "\n", what, q, a, b);
  return false;
}

static u64 g_rng = 0x9E3779B97F4A7C15ULL;
static u64 next_u64() {   // splitmix64
  u64 z = (g_rng += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

static u64 ref_mod(u128 x, u64 q) { return (u64)(x % q); }
static u64 ref_mulmod(u64 a, u64 b, u64 q) { return ref_mod((u128)a * b, q); }
static u64 ref_pow(u64 b, u64 e, u64 q) {
  u64 r = 1 % q;
  b %= q;
  for (; e; e >>= 1, b = ref_mulmod(b, b, q))
    if (e & 1) r = ref_mulmod(r, b, q);
  return r;
}

static std::vector<u64> operands(u64 q) {
  std::vector<u64> v = {0, 1, 2, q - 1, q, q + 1, 2 * q - 1, 2 * q, 3 * q - 1, (1ULL << 62) - 1, 1ULL << 62, (1ULL << 63) - 1,
                        1ULL << 63, ~0ULL, ~0ULL - 1, (u64)INT64_MIN, (u64)INT64_MAX, 0xFFFFFFFFULL, 0x100000000ULL,
                        0x8080808080808080ULL, 0x7F7F7F7F7F7F7F7FULL};
  for (int i = 0; i < 48; ++i) v.push_back(next_u64());
  for (int i = 0; i < 24; ++i) v.push_back(next_u64() % q);
  for (int i = 0; i < 8; ++i) v.push_back(next_u64() >> (next_u64() % 64));
  return v;
}

static void check_scalar_ops(u64 q, const Mod& m, const std::vector<u64>& ops) {
  for (u64 a : ops)
    for (u64 b : ops) {
      check(reduce128(a, b, m) == ref_mod(((u128)b << 64) | a, q), "reduce128", q, a, b);
      check(mulmod(a, b, m) == ref_mulmod(a, b, q), "mulmod", q, a, b);
    }
  // Shoup multiplication: every w < q, any 64-bit a
  std::vector<u64> ws = {0, 1, q - 1, q / 2, (q + 1) / 2};
  for (int i = 0; i < 8; ++i) ws.push_back(next_u64() % q);
  for (u64 w : ws) {
    const u64 wp = shoup_precompute(w, q);
    for (u64 a : ops) check(mulmod_shoup(a, w, wp, q) == ref_mulmod(a, w, q), "mulmod_shoup", q, a, w);
  }
  for (u64 a : ops) {
    const i64 c = (i64)a;
    const __int128 r = ((__int128)c % (__int128)q + q) % q;
    check(signed_residue(c, m) == (u64)r, "signed_residue", q, a);
  }
  check(powmod(3, q - 1, m) == 1, "powmod", q);   // Fermat: q is prime and 3 < q or 3 = 0 mod q never happens for q > 3
}

// the digit step of vec_digits_kernel / vec_digits7_kernel: y, y 256, y 256^2, ... mod q, one Shoup multiply each
static void check_digit_step(u64 q, const Mod& m, const std::vector<u64>& ops) {
  u64 w, wp;
#if defined(PVW_PARENT_DIGIT_STEP)
  w = 256;
  wp = (m.ratio_hi << 8) | (m.ratio_lo >> 56);
#else
  mul256_consts(m, w, wp);
  check(w < q && w == ref_mod(256, q), "mul256_consts.w", q, w);
  check(wp == shoup_precompute(w, q), "mul256_consts.wp", q, wp);
  if (q > 256) check(w == 256 && wp == ((m.ratio_hi << 8) | (m.ratio_lo >> 56)), "mul256_consts.unchanged", q, wp);
#endif
  for (u64 y : ops) {
    if (y >= q) continue;   // the kernels step reduced residues
    u64 cur = y, want = y;
    for (int a = 0; a < 8; ++a) {
      if (!check(cur == want, "digit_step", q, y, (u64)a)) break;
      cur = mulmod_shoup(cur, w, wp, q);
      want = ref_mulmod(want, 256, q);
    }
  }
  for (u64 y = 0; y < q && y < 1024; ++y) {   // every residue of the small moduli
    u64 cur = y, want = y;
    for (int a = 0; a < 8; ++a) {
      if (!check(cur == want, "digit_step", q, y, (u64)a)) break;
      cur = mulmod_shoup(cur, w, wp, q);
      want = ref_mulmod(want, 256, q);
    }
  }
}

// acc_mac / acc_add / acc_reduce against the sum of the products mod q, up to 2^32 terms of the largest products
static u64 ref_acc(const Acc& a, u64 q) {
  const u64 t64 = ref_mod((u128)1 << 64, q);           // 2^64 mod q
  const u64 t32 = ref_mod((u128)1 << 32, q);
  const u64 t96 = ref_mulmod(t64, t32, q), t128 = ref_mulmod(t64, t64, q);
  u128 s = 0;
  auto add = [&](u64 v, u64 wgt) { s = (s + ref_mulmod(v % q, wgt, q)) % q; };
  add(a.ll, 1);
  add(a.cll, t64);
  add(a.lh, t32);
  add(a.hl, t32);
  add(a.clh, t96);
  add(a.chl, t96);
  add(a.hh, t64);
  add(a.chh, t128);
  return (u64)s;
}

static void preload(Acc& a, u64 nterms) {   // the state after nterms products (2^64 - 1)^2
  const u128 part = (u128)0xFFFFFFFFULL * 0xFFFFFFFFULL;   // each 32x32 partial product
  const u128 tot = part * nterms;                           // < 2^96
  a.ll = a.lh = a.hl = a.hh = (u64)tot;
  a.cll = a.clh = a.chl = a.chh = (u32)(tot >> 64);
}

static void check_acc(u64 q, const Mod& m, const std::vector<u64>& ops) {
  const u64 maxsq = ref_mulmod(~0ULL, ~0ULL, q);
  {   // random operands
    Acc a;
    acc_zero(a);
    u64 want = 0;
    for (size_t i = 0; i < ops.size(); ++i) {
      const u64 x = ops[i], y = ops[(i * 7 + 3) % ops.size()];
      acc_mac(a, x, y);
      want = (want + ref_mulmod(x, y, q)) % q;
    }
    check(acc_reduce(a, m) == want, "acc_mac", q);
    check(ref_acc(a, q) == want, "acc_ref", q);
  }
  // the bound the header claims: 2^32 terms of the largest products (wrap counters preloaded), split over two
  // accumulators that acc_add joins (the cross-wave reduction)
  for (u64 tail : {0ULL, 1ULL, 5ULL, 64ULL}) {
    const u64 total = 1ULL << 32, n1 = (total - tail) / 3, n2 = total - tail - n1;
    Acc a, b;
    acc_zero(a);
    acc_zero(b);
    preload(a, n1);
    preload(b, n2);
    for (u64 i = 0; i < tail; ++i) acc_mac(i & 1 ? a : b, ~0ULL, ~0ULL);
    check(ref_acc(a, q) == ref_mulmod(n1 + tail / 2, maxsq, q), "acc_preload", q, n1, tail);   // a took the odd i
    acc_add(a, b);
    check(acc_reduce(a, m) == ref_mulmod(total, maxsq, q), "acc_bound", q, total, tail);
  }
  {   // one term of every operand pair after a preload to 2^32 - 64 terms
    Acc a;
    acc_zero(a);
    preload(a, (1ULL << 32) - 64);
    u64 want = ref_mulmod((1ULL << 32) - 64, maxsq, q);
    for (int i = 0; i < 64; ++i) {
      const u64 x = ops[(size_t)i % ops.size()], y = ops[(size_t)(i * 5 + 1) % ops.size()];
      acc_mac(a, x, y);
      want = (want + ref_mulmod(x, y, q)) % q;
    }
    check(acc_reduce(a, m) == want, "acc_mixed_bound", q);
  }
}

template <int L_>
static void check_ntt(u64 q, const Mod& m) {
  if ((q - 1) % (2 * L_) != 0) return;
  u64 psi = 0;   // an element of order exactly 2l: psi^l = -1
  for (u64 g = 2; g < q && !psi; ++g) {
    const u64 c = ref_pow(g, (q - 1) / (2 * L_), q);
    if (ref_pow(c, L_, q) == q - 1) psi = c;
  }
  if (!check(psi != 0, "ntt.root", q)) return;
  const u64 ipsi = ref_pow(psi, q - 2, q);
  u32 bits = 0;
  while ((1 << bits) < L_) ++bits;
  u64 tw[L_], twp[L_], itw[L_], itwp[L_];
  for (int i = 0; i < L_; ++i) {
    tw[i] = ref_pow(psi, bitrev32(i, bits), q);
    twp[i] = shoup_precompute(tw[i], q);
    itw[i] = ref_pow(ipsi, bitrev32(i, bits), q);
    itwp[i] = shoup_precompute(itw[i], q);
  }
  const u64 linv = ref_pow(L_, q - 2, q), linvp = shoup_precompute(linv, q);
  for (int t = 0; t < 6; ++t) {
    u64 a[L_], orig[L_];
    for (int j = 0; j < L_; ++j) {
      const u64 r = next_u64() % q;
      orig[j] = a[j] = t == 0 ? 0 : t == 1 ? q - 1 : t == 2 ? (j == 0 ? 1 : 0) : r;
    }
    ntt_forward<L_>(a, tw, twp, m);
    bool ok = true;
    for (int s = 0; s < L_; ++s) {
      const u64 x = ref_pow(psi, 2 * bitrev32(s, bits) + 1, q);
      u64 v = 0, xp = 1;
      for (int j = 0; j < L_; ++j) {
        v = (v + ref_mulmod(orig[j], xp, q)) % q;
        xp = ref_mulmod(xp, x, q);
      }
      ok = ok && a[s] == v;
    }
    check(ok, L_ == 8 ? "ntt_forward.8" : L_ == 16 ? "ntt_forward.16" : L_ == 32 ? "ntt_forward.32" : "ntt_forward.64", q);
    ntt_inverse<L_>(a, itw, itwp, linv, linvp, m);
    ok = true;
    for (int j = 0; j < L_; ++j) ok = ok && a[j] == orig[j];
    check(ok, L_ == 8 ? "ntt_inverse.8" : L_ == 16 ? "ntt_inverse.16" : L_ == 32 ? "ntt_inverse.32" : "ntt_inverse.64", q);
  }
}

// the unreduced word classes of the residue-word contract (include/pvw_hip.h): w means w mod q for any 64-bit w
static std::vector<u64> raw_words(u64 q) {
  const u64 w = next_u64() % q;
  std::vector<u64> v = {q - 1, q, 2 * q - 1, w + q, w + (~0ULL - w) / q * q, (1ULL << 56) - 1, 1ULL << 56, 1ULL << 61,
                        1ULL << 62, (1ULL << 63) - (1ULL << 55) - 1, (1ULL << 63) - (1ULL << 55), 1ULL << 63, 0 - q, ~0ULL};
  for (int i = 0; i < 16; ++i) v.push_back(next_u64());
  return v;
}

static u64 load_word(u64 w, const Mod& m) {   // what a kernel does with a caller's word at its load
#ifdef PVW_RAW_WORDS
  (void)m;
  return w;
#else
  return reduce_word(w, m);
#endif
}

static void check_reduce_word(u64 q, const Mod& m, const std::vector<u64>& ops) {
  std::vector<u64> ws = raw_words(q);
  ws.insert(ws.end(), ops.begin(), ops.end());
  for (u64 w : ws) check(reduce_word(w, m) == w % q, "reduce_word", q, w);
  // the balanced base-256 digits of the GEMM operands ((w + C) ^ C, vec_digits_kernel) rebuild the loaded word exactly
  const u64 C = 0x8080808080808080ULL;
  for (u64 w : ws) {
    const u64 x = load_word(w, m), d = (x + C) ^ C;
    __int128 v = 0;
    for (int b = 7; b >= 0; --b) v = v * 256 + (signed char)(d >> (8 * b));
    check(v >= 0 && (u64)v % q == w % q, "raw_words.digits", q, w);
  }
}

// an l-point NTT of rows of unreduced words (one class per row, and rows mixing them) against the transform of the words
// reduced: every slot below q and equal
template <int L_>
static void check_ntt_raw(u64 q, const Mod& m) {
  if ((q - 1) % (2 * L_) != 0) return;
  u64 psi = 0;
  for (u64 g = 2; g < q && !psi; ++g) {
    const u64 c = ref_pow(g, (q - 1) / (2 * L_), q);
    if (ref_pow(c, L_, q) == q - 1) psi = c;
  }
  if (!psi) return;
  const u64 ipsi = ref_pow(psi, q - 2, q);
  u32 bits = 0;
  while ((1 << bits) < L_) ++bits;
  u64 tw[L_], twp[L_], itw[L_], itwp[L_];
  for (int i = 0; i < L_; ++i) {
    tw[i] = ref_pow(psi, bitrev32(i, bits), q);
    twp[i] = shoup_precompute(tw[i], q);
    itw[i] = ref_pow(ipsi, bitrev32(i, bits), q);
    itwp[i] = shoup_precompute(itw[i], q);
  }
  const u64 linv = ref_pow(L_, q - 2, q), linvp = shoup_precompute(linv, q);
  const std::vector<u64> ws = raw_words(q);
  const char* fw = L_ == 8 ? "raw_words.ntt_forward.8" : L_ == 16 ? "raw_words.ntt_forward.16" : L_ == 32 ? "raw_words.ntt_forward.32" : "raw_words.ntt_forward.64";
  const char* iv = L_ == 8 ? "raw_words.ntt_inverse.8" : L_ == 16 ? "raw_words.ntt_inverse.16" : L_ == 32 ? "raw_words.ntt_inverse.32" : "raw_words.ntt_inverse.64";
  for (size_t row = 0; row < ws.size() + 4; ++row) {
    u64 raw[L_], a[L_], b[L_], ra[L_], rb[L_];
    for (int j = 0; j < L_; ++j) raw[j] = row < ws.size() ? ws[row] - (u64)j * (row & 1) : ws[(row + 3 * j) % ws.size()];
    for (int j = 0; j < L_; ++j) {
      a[j] = b[j] = load_word(raw[j], m);
      ra[j] = rb[j] = raw[j] % q;
    }
    ntt_forward<L_>(a, tw, twp, m);
    ntt_forward<L_>(ra, tw, twp, m);
    ntt_inverse<L_>(b, itw, itwp, linv, linvp, m);
    ntt_inverse<L_>(rb, itw, itwp, linv, linvp, m);
    bool okf = true, oki = true;
    for (int s = 0; s < L_; ++s) {
      okf = okf && a[s] == ra[s] && a[s] < q;
      oki = oki && b[s] == rb[s] && b[s] < q;
    }
    check(okf, fw, q, raw[0]);
    check(oki, iv, q, raw[0]);
  }
}

int main() {
  std::vector<u64> moduli;
  unsigned long long q;
  while (scanf("%llu", &q) == 1) moduli.push_back(q);
  for (u64 qq : moduli) {
    const Mod m = make_mod(qq);
    const std::vector<u64> ops = operands(qq);
    check_digit_step(qq, m, ops);
    check_scalar_ops(qq, m, ops);
    check_acc(qq, m, ops);
    check_ntt<8>(qq, m);
    check_ntt<16>(qq, m);
    check_ntt<32>(qq, m);
    check_ntt<64>(qq, m);
    check_reduce_word(qq, m, ops);
    check_ntt_raw<8>(qq, m);
    check_ntt_raw<16>(qq, m);
    check_ntt_raw<32>(qq, m);
    check_ntt_raw<64>(qq, m);
  }
  if (g_fail) return 1;
  printf("ARITH_EDGES_OK %zu\n", moduli.size());
  return 0;
}

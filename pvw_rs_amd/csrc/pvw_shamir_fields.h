// pvw_shamir_fields.h -- host only: the two fields of the Shamir reconstruction entry points (DESIGN "Reconstruction entry
// points") as far as a call's shape and scratch go, and the layouts and sizing rules that both run through.  No HIP
// declaration is needed here, so a program of the host compiler can include it (tests/cpp/shamir_layouts.cpp); what a driver
// needs on top -- the kernels' parameter blocks, launchers, scope names and messages -- is added in pvw_capi.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pvw_wide.h"

namespace pvw {

// One word per element, p < 2^64.  The three word counts are the kernels' (pvw_kernels.h:
// shamir_interp_words, shamir_correct_public_words, shamir_evaluate_public_words): declared here, defined where those are seen.
struct NarrowField {
  static constexpr size_t EW = 1;                        // words per element
  typedef u64 Modulus;                                   // how a call names p
  struct HostMod {};
  static size_t interp_words(size_t count, u32 t);
  static size_t correct_public_words(size_t count, u32 t, size_t nk);
  static size_t evaluate_public_words(size_t count, size_t Tg, size_t nk);
  static size_t up(size_t w) { return w; }               // where a region of elements may start
  static constexpr size_t kNeedSlack = 16;               // what evaluate_need_bytes adds for the two u32 rows' roundings
  // The per-secret scratch of the evaluation, in bytes: a row of M, of the syndromes and of the locators as in correct_piece, and
  // a row of y o M, of raw, of Lambda and of Lambda' at the group's targets, a stand-in for out, L and a stand-in for nerr
  static size_t evaluate_secret_bytes(size_t count, size_t red, size_t nk, size_t Tg) { return (2 * count + red + nk + 3 * Tg + 2) * 8; }
};
// Four words per element, p < 2^256; the word counts are shamir_interp_wide_words and so on.
struct WideField {
  static constexpr size_t EW = 4;
  typedef const u64* Modulus;                            // [4], host
  typedef WideMod HostMod;                               // set by reconstruct_wide_checks
  static size_t interp_words(size_t count, u32 t);
  static size_t correct_public_words(size_t count, u32 t, size_t nk);
  static size_t evaluate_public_words(size_t count, size_t Tg, size_t nk);
  static size_t up(size_t w) { return (w + 3) & ~(size_t)3; }   // every region of elements starts at a multiple of four words
  static constexpr size_t kNeedSlack = 96;               // covers the layout's roundings
  // ... the rows as above with elements of 32 bytes and a stand-in for out; L and a stand-in for nerr
  static size_t evaluate_secret_bytes(size_t count, size_t red, size_t nk, size_t Tg) { return (2 * count + red + nk + 3 * Tg + 1) * 32 + 8; }
};

// One call.  The basis columns 0..t give F_s; out[s] = F_s(0); every extra column is compared with F_s at its point.
template <class F>
struct Reconstruct {
  typename F::Modulus p;
  u32 degree;
  const u64* indices;   // [count], host
  size_t count, S, secret_stride, point_stride;
  bool erasures = false;   // a call with an erasure mask: the locator of a row has up to r + 1 coefficients
  typename F::HostMod m{};
  size_t T() const { return count - degree; }
  size_t red() const { return count - degree - 1; }
  size_t nk() const { return erasures ? red() + 1 : red() / 2 + 1; }   // the locator capacity of the corrected decode
  size_t ws_bytes() const { return F::interp_words(count, degree) * 8; }
};

// The device scratch of one corrected call, in words from its base: M first (the one region marked secret besides the staging),
// then what the indices alone decide, then what the errors decide.  `cap` secrets are in flight at a time.
//   M [cap][count][EW] | x, aux, lambda, V, X (correct_public_words) | Synd [cap][r][EW] | Lambda [cap][nk][EW] | L [cap] (u32)
// nk, the locator capacity, is E + 1, or r + 1 for a call with erasures: X has nk rows as well.  Every offset is a multiple of EW.
template <class F>
struct CorrectLayout {
  size_t count, r, nk, cap;
  size_t pub, synd, lam, L, total;   // word offsets
  CorrectLayout(const Reconstruct<F>& rc, size_t cap_) : count(rc.count), r(rc.red()), nk(rc.nk()), cap(cap_) {
    pub = cap * count * F::EW;
    synd = pub + F::correct_public_words(count, rc.degree, nk);
    lam = synd + cap * r * F::EW;
    L = lam + cap * nk * F::EW;
    total = L + (cap + 1) / 2;
  }
  size_t bytes() const { return total * 8; }
  size_t m_bytes() const { return cap * count * F::EW * 8; }
};
// Secrets per pass over the kernels: their per-secret scratch (a row of M, of the syndromes and of the locators) stays
// within `budget` -- 64 MiB; M alone is count elements a secret -- and within what one grid holds.
inline size_t pass_cap(size_t budget, size_t per, size_t S) {
  size_t cap = budget / per;
  if (cap == 0) cap = 1;
  if (cap > 65535u * 4) cap = 65535u * 4;
  return cap < S ? cap : S;
}
template <class F>
size_t correct_piece(const Reconstruct<F>& r, size_t budget) {
  return pass_cap(budget, (r.count + r.red() + r.nk()) * F::EW * 8 + 4, r.S);
}

// Targets per group: the public matrices that depend on the targets (a column of C, of Xt and of Xd, scale and coin per target)
// stay within `budget` -- 64 MiB; at count = T = 4096, t = 2047 the one-word ones would be 134 MB + 2 x 34 MB in one piece.
// Whole blocks of 64 targets when there are that many.
template <class F>
size_t evaluate_group(const Reconstruct<F>& r, size_t num_targets, size_t budget) {
  size_t tg = budget / ((r.count + 2 * r.nk() + 2) * F::EW * 8 + 4);
  if (tg > 64) tg -= tg % 64;
  if (tg == 0) tg = 1;
  return tg < num_targets ? tg : num_targets;
}
template <class F>
size_t evaluate_secret_bytes(const Reconstruct<F>& r, size_t Tg) {
  return F::evaluate_secret_bytes(r.count, r.red(), r.nk(), Tg);
}
// secrets per pass, by the rule of correct_piece
template <class F>
size_t evaluate_piece(const Reconstruct<F>& r, size_t Tg, size_t budget) {
  return pass_cap(budget, evaluate_secret_bytes(r, Tg), r.S);
}
// The scratch of one evaluation, in words from its base: the block of the corrected call first (CorrectLayout: M leads it), then
//   YM [cap][count][EW] | raw [cap][Tg][EW] | outs [cap][EW]   -- depend on the shares: the second region marked secret
//   LamT [cap][Tg][EW] | LamD [cap][Tg][EW] | nerr [cap] (u32) | the group's public matrices (evaluate_public_words)
// Every region of elements starts at a multiple of EW words (F::up).
template <class F>
struct EvaluateLayout {
  CorrectLayout<F> cl;
  size_t Tg;
  size_t ym, raw, outs, lamT, lamD, nerr, pub, total;   // word offsets
  EvaluateLayout(const Reconstruct<F>& rc, size_t cap, size_t Tg_) : cl(rc, cap), Tg(Tg_) {
    ym = F::up(cl.total);
    raw = ym + cap * rc.count * F::EW;
    outs = raw + cap * Tg * F::EW;
    lamT = outs + cap * F::EW;
    lamD = lamT + cap * Tg * F::EW;
    nerr = lamD + cap * Tg * F::EW;
    pub = F::up(nerr + (cap + 1) / 2);
    total = pub + F::evaluate_public_words(rc.count, Tg, cl.nk);
  }
  size_t bytes() const { return total * 8; }
  size_t secret_bytes() const { return (lamT - ym) * 8; }
};
// What the stream's block must hold for a call: never less than the layout takes, and no smaller for more secrets or more
// targets at the same (degree, count), nor with a mask -- the rule a captured call is checked by.
template <class F>
size_t evaluate_need_bytes(const Reconstruct<F>& r, size_t Tg, size_t budget) {
  const size_t per = evaluate_secret_bytes(r, Tg);
  size_t part = r.S > budget / per ? budget : r.S * per;
  if (part < per) part = per;
  return part + F::kNeedSlack + (F::correct_public_words(r.count, r.degree, r.nk()) + F::evaluate_public_words(r.count, Tg, r.nk())) * 8;
}

}  // namespace pvw

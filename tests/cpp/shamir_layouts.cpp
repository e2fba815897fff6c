// The scratch layouts and sizing rules of the Shamir reconstruction entry points (pvw_shamir_fields.h), for both fields, against
// the formulas the one-word and the 256-bit drivers each carried before they were folded, written out here literally.  What a call
// allocates, where each region starts and when a captured call counts as sized depend on nothing else, so this pins them without
// a GPU.  A program of its own, built with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "pvw_shamir_fields.h"

using namespace pvw;

// the kernels' word counts (pvw_kernels.h), which a host-only program states itself
size_t NarrowField::interp_words(size_t count, u32 t) { return 2 * count + 1 + ((size_t)t + 1) * (count - t); }
size_t NarrowField::correct_public_words(size_t count, u32 t, size_t nk) { return 3 * count + 1 + count * (count - t - 1) + nk * count; }
size_t NarrowField::evaluate_public_words(size_t count, size_t Tg, size_t nk) { return 2 * Tg + count * Tg + 2 * nk * Tg + (Tg + 1) / 2; }
size_t WideField::interp_words(size_t count, u32 t) { return 4 * (2 * count + 1 + ((size_t)t + 1) * (count - t)); }
size_t WideField::correct_public_words(size_t count, u32 t, size_t nk) { return 4 * (3 * count + 1 + count * (count - t - 1) + nk * count); }
size_t WideField::evaluate_public_words(size_t count, size_t Tg, size_t nk) { return 4 * (2 * Tg + count * Tg + 2 * nk * Tg) + (Tg + 1) / 2; }

static long g_checks = 0;
#define CHECK(a, b)                                                                                                        \
  do {                                                                                                                     \
    ++g_checks;                                                                                                            \
    if ((size_t)(a) != (size_t)(b)) {                                                                                      \
      printf("MISMATCH %s = %zu, %s = %zu (count %zu degree %u erasures %d S %zu cap %zu Tg %zu budget %zu) at line %d\n", \
             #a, (size_t)(a), #b, (size_t)(b), count, degree, (int)erasures, S, cap, Tg, budget, __LINE__);                \
      exit(1);                                                                                                             \
    }                                                                                                                      \
  } while (0)

static size_t clamp_cap(size_t cap, size_t S) {
  if (cap == 0) cap = 1;
  if (cap > 65535u * 4) cap = 65535u * 4;
  return cap < S ? cap : S;
}
static size_t up4(size_t w) { return (w + 3) & ~(size_t)3; }

template <class F>
static void one(size_t count, u32 degree, bool erasures, size_t S, size_t cap, size_t Tg, size_t budget) {
  constexpr bool wide = F::EW == 4;
  Reconstruct<F> r{};
  r.degree = degree, r.count = count, r.S = S, r.secret_stride = count, r.point_stride = 1, r.erasures = erasures;
  const size_t red = count - degree - 1, nk = erasures ? red + 1 : red / 2 + 1;
  CHECK(r.red(), red);
  CHECK(r.nk(), nk);
  CHECK(r.T(), count - degree);
  const size_t cpub = wide ? 4 * (3 * count + 1 + count * red + nk * count) : 3 * count + 1 + count * red + nk * count;
  const size_t epub = wide ? 4 * (2 * Tg + count * Tg + 2 * nk * Tg) + (Tg + 1) / 2 : 2 * Tg + count * Tg + 2 * nk * Tg + (Tg + 1) / 2;
  CHECK(r.ws_bytes(), (wide ? 4 : 1) * (2 * count + 1 + ((size_t)degree + 1) * (count - degree)) * 8);

  // CorrectLayout | CorrectWideLayout
  const CorrectLayout<F> cl(r, cap);
  size_t pub, synd, lam, L, total;
  if (!wide) {
    pub = cap * count;
    synd = pub + cpub;
    lam = synd + cap * red;
    L = lam + cap * nk;
    total = L + (cap + 1) / 2;
    CHECK(cl.m_bytes(), cap * count * 8);
  } else {
    pub = cap * count * 4;
    synd = pub + cpub;
    lam = synd + cap * red * 4;
    L = lam + cap * nk * 4;
    total = L + (cap + 1) / 2;
    CHECK(cl.m_bytes(), cap * count * 32);
  }
  CHECK(cl.pub, pub);
  CHECK(cl.synd, synd);
  CHECK(cl.lam, lam);
  CHECK(cl.L, L);
  CHECK(cl.total, total);
  CHECK(cl.bytes(), total * 8);
  CHECK(cl.count, count);
  CHECK(cl.r, red);
  CHECK(cl.nk, nk);
  CHECK(cl.cap, cap);

  // EvaluateLayout | EvaluateWideLayout
  const EvaluateLayout<F> el(r, cap, Tg);
  size_t ym, raw, outs, lamT, lamD, nerr, epubo, etotal;
  if (!wide) {
    ym = total;
    raw = ym + cap * count;
    outs = raw + cap * Tg;
    lamT = outs + cap;
    lamD = lamT + cap * Tg;
    nerr = lamD + cap * Tg;
    epubo = nerr + (cap + 1) / 2;
    etotal = epubo + epub;
  } else {
    ym = up4(total);
    raw = ym + cap * count * 4;
    outs = raw + cap * Tg * 4;
    lamT = outs + cap * 4;
    lamD = lamT + cap * Tg * 4;
    nerr = lamD + cap * Tg * 4;
    epubo = up4(nerr + (cap + 1) / 2);
    etotal = epubo + epub;
  }
  CHECK(el.cl.total, total);
  CHECK(el.Tg, Tg);
  CHECK(el.ym, ym);
  CHECK(el.raw, raw);
  CHECK(el.outs, outs);
  CHECK(el.lamT, lamT);
  CHECK(el.lamD, lamD);
  CHECK(el.nerr, nerr);
  CHECK(el.pub, epubo);
  CHECK(el.total, etotal);
  CHECK(el.bytes(), etotal * 8);
  CHECK(el.secret_bytes(), (lamT - ym) * 8);
  if (wide)   // every region of elements starts at a multiple of four words
    for (size_t off : {cl.pub, cl.synd, cl.lam, cl.L, el.ym, el.raw, el.outs, el.lamT, el.lamD, el.pub}) CHECK(off % 4, 0);

  // correct_piece | correct_wide_piece
  CHECK(correct_piece(r, budget), clamp_cap(budget / ((count + red + nk) * (wide ? 32 : 8) + 4), S));
  // evaluate_group | evaluate_wide_group, with Tg targets asked for and with many
  for (size_t num_targets : {Tg, (size_t)100000}) {
    size_t tg = budget / ((count + 2 * nk + 2) * (wide ? 32 : 8) + 4);
    if (tg > 64) tg -= tg % 64;
    if (tg == 0) tg = 1;
    CHECK(evaluate_group(r, num_targets, budget), tg < num_targets ? tg : num_targets);
  }
  // evaluate_secret_bytes | evaluate_wide_secret_bytes
  const size_t per = wide ? (2 * count + red + nk + 3 * Tg + 1) * 32 + 8 : (2 * count + red + nk + 3 * Tg + 2) * 8;
  CHECK(evaluate_secret_bytes(r, Tg), per);
  // evaluate_piece | evaluate_wide_piece
  CHECK(evaluate_piece(r, Tg, budget), clamp_cap(budget / per, S));
  // evaluate_need_bytes | evaluate_wide_need_bytes
  size_t part = S > budget / per ? budget : S * per;
  if (part < per) part = per;
  const size_t need = part + (wide ? 96 : 16) + (cpub + epub) * 8;
  CHECK(evaluate_need_bytes(r, Tg, budget), need);
  // what the evaluation's device call asks of its own numbers ("layout beyond its bound"): the layout of the pass it runs fits
  const EvaluateLayout<F> run(r, evaluate_piece(r, Tg, budget), Tg);
  ++g_checks;
  if (need < run.bytes()) {
    printf("LAYOUT BEYOND ITS BOUND need %zu bytes %zu (EW %zu count %zu degree %u erasures %d S %zu Tg %zu budget %zu)\n", need, run.bytes(),
           (size_t)F::EW, count, degree, (int)erasures, S, Tg, budget);
    exit(1);
  }
  // ... and the layout of `cap` secrets, which is the pass of a call with S = cap under a budget that holds them
  if (S == cap && budget / per >= cap) CHECK(run.bytes(), etotal * 8);
}

int main() {
  long cases = 0;
  const size_t counts[] = {1, 2, 7, 64, 65, 4096};
  for (size_t count : counts) {
    const size_t degrees[] = {0, 2, count - 1};
    for (int d = 0; d < 3; ++d) {
      const size_t degree = degrees[d];
      if (degree > count - 1 || (d == 2 && (degree == 0 || degree == 2))) continue;   // a degree the count cannot have, or one seen
      for (int erasures = 0; erasures < 2; ++erasures)
        for (size_t cap : {1, 2, 5})
          for (size_t Tg : {1, 2, 3, 64})
            // S: the layout's own cap, one secret, more than one grid holds; budgets: the shipped 64 MiB, one that holds two
            // secrets or two targets of the narrow field at this shape, and one that holds nothing
            for (size_t S : {cap, (size_t)1, (size_t)65535 * 4 + 7})
              for (size_t budget : {(size_t)64 << 20, 2 * ((2 * count + 2 * (count - degree) + 3 * Tg + 2) * 8) + 8, (size_t)1}) {
                one<NarrowField>(count, (u32)degree, erasures != 0, S, cap, Tg, budget);
                one<WideField>(count, (u32)degree, erasures != 0, S, cap, Tg, budget);
                cases += 2;
              }
    }
  }
  printf("SHAMIR_LAYOUTS_OK cases %ld checks %ld\n", cases, g_checks);
  return 0;
}

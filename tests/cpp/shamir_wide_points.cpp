// The evaluation of the corrected polynomials at FIELD POINTS over a prime below 2^256: the kernels behind
// pvw_shamir_evaluate_wide_*_at* and pvw_shamir_packed_wide_secrets* on the ground 8.22 never gave them -- the point 0, points
// above 2^64 (p - 1, p - 2, the packed secret points p - m) and points that meet a column without being a target's index + 1.
// The restatement of the kernels is that of shamir_wide_evaluate.cpp, taken as it is (its decode, y o M, scale / coin, Cauchy
// entries, Xt, Xd, the three products and the finish rule, sequentially over pvw_wide.h); restated here are the two ways a point
// reaches them -- shamir_points_from_wide_kernel (wide_mont_in of the words) and shamir_packed_secret_points_wide_kernel
// (wide_mont_in of m, then the negation, m = 0 giving 0) -- which must agree.  Checked against Horner's rule on the polynomial
// that Berlekamp-Welch finds on the sub-row of the columns that are not erased, and at the point 0 against the decode's secret.
// Stand-alone: shamir_wide_points <prime in hex>...
#define main shamir_wide_evaluate_main
#include "shamir_wide_evaluate.cpp"
#undef main

// shamir_packed_secret_points_wide_kernel, thread i of a launch at m0
static W4 packed_point(u32 m0, u32 i, const WideMont& m) {
  const u64 mw[4] = {(u64)m0 + i, 0, 0, 0};
  W4 mr, v = {{0, 0, 0, 0}};
  wide_mont_in(mw, m, mr.v);
  wide_sub_p(v.v, mr.v, m);
  return v;
}
// shamir_points_from_wide_kernel on the words of p - k (k = 0 stands for the point 0)
static W4 field_point(const u64 (&p)[4], u64 k, const WideMont& m) {
  u64 w[4] = {0, 0, 0, 0};
  if (k) {
    u64 br = k;
    for (int i = 0; i < 4; ++i) {
      w[i] = p[i] - br;
      br = p[i] < br;
    }
  }
  W4 v;
  wide_mont_in(w, m, v.v);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  long decodable = 0, undecodable = 0, checked = 0, at_zero = 0, on_columns = 0;
  for (int a = 1; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p) || !(p[0] & 1)) return 2;
    const WideMont m = make_wide_mont(p);
    rng_state = 0x25A7E500 + (u64)a;
    if (!(p[1] | p[2] | p[3]) && p[0] <= 65000) return 2;        // the columns' points come from 1 .. 60000, the packed ones from above
    const u64 pool = 60000;
    const u32 KMAX = 70;                                         // beyond one 64-point batch
    for (u32 i = 0; i < KMAX; ++i) {
      const W4 g = packed_point(i < 64 ? 0 : 64, i < 64 ? i : i - 64, m), w = field_point(p, i, m);   // two groups of a launch
      if (memcmp(g.v, w.v, 32) != 0 || (i == 0 && !is0(g))) {
        printf("POINT MISMATCH prime %s m %u\n", argv[a], i);
        return 1;
      }
    }
    struct Shape { u32 t, r, eps, nu; };
    std::vector<Shape> shapes;
    for (u32 t = 0; t < 3; ++t)
      for (u32 r = 0; r < 6; ++r)
        for (u32 eps = 0; eps <= r + 1; ++eps) {
          const u32 Es = eps <= r ? (r - eps) / 2 : 0;
          for (u32 nu = 0; nu <= Es + 1 && eps + nu <= t + 1 + r; ++nu) shapes.push_back({t, r, eps, nu});
        }
    for (size_t i = 0; i < shapes.size(); ++i) {
      const u32 t = shapes[i].t, r = shapes[i].r, eps = shapes[i].eps, nu = shapes[i].nu, count = t + 1 + r;
      const u32 K = i % 64 == 0 ? KMAX : 1 + (u32)(i % 5);       // the packed points 0, p - 1, .., p - (K - 1)
      std::vector<W4> x(count), y(count), co(t + 1);
      std::vector<u64> pts;
      while (pts.size() < count) {
        const u64 v = 1 + rnd64() % pool;                        // far below p - K: no packed point meets a column
        bool dup = false;
        for (u64 q : pts) dup |= q == v;
        if (!dup) pts.push_back(v);
      }
      for (u32 c = 0; c < count; ++c) {
        const u64 xw[4] = {pts[c], 0, 0, 0};
        wide_mont_in(xw, m, x[c].v);
      }
      for (u32 j = 0; j <= t; ++j) {
        const u64 w[4] = {rnd64(), rnd64(), rnd64(), rnd64()};
        wide_mont_in(w, m, co[j].v);
      }
      for (u32 c = 0; c < count; ++c) {
        W4 v = co[t];
        for (u32 j = t; j-- > 0;) v = add(mul(v, x[c], m), co[j], m);
        wide_mont_out(v.v, m, y[c].v);
      }
      std::vector<u32> pick;
      while (pick.size() < eps + nu) {
        const u32 c = (u32)(rnd64() % count);
        bool dup = false;
        for (u32 q : pick) dup |= q == c;
        if (!dup) pick.push_back(c);
      }
      std::vector<bool> er(count, false);
      for (u32 k = 0; k < eps + nu; ++k) {
        const u32 c = pick[k];
        if (k < eps) {
          er[c] = true;
          for (int w = 0; w < 4; ++w) y[c].v[w] = k % 2 ? rnd64() : ~(u64)0;
        } else {
          y[c].v[rnd64() % 4] ^= (u64)1 << (rnd64() % 64);
        }
      }
      std::vector<W4> psi, M, u, F;
      const Report got = kernel_decode(x, y, er, t, m, psi, M, u), want = contract(x, y, er, t, m, F);
      if (!(got == want)) {
        printf("MISMATCH prime %s shape %zu (t %u r %u eps %u nu %u): nerr %u / %u\n", argv[a], i, t, r, eps, nu, got.nerr, want.nerr);
        return 1;
      }
      // the points: the packed ones 0, p - 1, .., p - (K - 1) as the packed kernel makes them; every column's point as a field
      // element (right, wrong and erased columns, in reverse order); p - 1 and 0 once more, from their words
      std::vector<W4> xt;
      for (u32 k = 0; k < K; ++k) xt.push_back(packed_point(0, k, m));
      for (u32 c = count; c-- > 0;) {
        const u64 xw[4] = {pts[c], 0, 0, 0};
        W4 v;
        wide_mont_in(xw, m, v.v);
        xt.push_back(v);
      }
      xt.push_back(field_point(p, 1, m));
      xt.push_back(field_point(p, 0, m));
      const std::vector<W4> values = kernel_evaluate(x, u, y, psi, M, got.nerr != UNDECODABLE, xt, m);
      for (size_t j = 0; j < xt.size(); ++j) {
        W4 v = {{0, 0, 0, 0}};
        if (want.nerr != UNDECODABLE) {
          v = F[t];
          for (u32 k = t; k-- > 0;) v = add(mul(v, xt[j], m), F[k], m);
          wide_mont_out(v.v, m, v.v);
        }
        if (memcmp(v.v, values[j].v, 32) != 0) {
          printf("VALUE MISMATCH prime %s shape %zu (t %u r %u eps %u nu %u) point %zu of %zu\n", argv[a], i, t, r, eps, nu, j, xt.size());
          return 1;
        }
        ++checked;
        on_columns += j >= K && j < K + count;
      }
      // the point 0 is the secret of the decode, at both places it stands
      if (memcmp(values[0].v, got.out.v, 32) != 0 || memcmp(values.back().v, got.out.v, 32) != 0) {
        printf("the value at 0 is not out: prime %s shape %zu\n", argv[a], i);
        return 1;
      }
      ++at_zero;
      (want.nerr == UNDECODABLE ? undecodable : decodable)++;
    }
  }
  if (!decodable || !undecodable || !on_columns) return 1;
  printf("SHAMIR_WIDE_POINTS_OK %ld decodable %ld undecodable, %ld values, %ld on columns, %ld at 0\n", decodable, undecodable, checked,
         on_columns, at_zero);
  return 0;
}

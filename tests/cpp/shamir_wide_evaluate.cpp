// The evaluation of the corrected polynomials over a prime below 2^256 (pvw_rs_amd/csrc/pvw_shamir.hip), restated
// sequentially in the kernels' update order and Montgomery forms over pvw_wide.h's own product, accumulator and reduction: behind
// the decode of 8.21 (restated as in shamir_wide_erasures.cpp) y o M by one REDC, the scale and the coinciding column of every
// target met over 64 lanes, the Cauchy entries with 32 differences per inversion running through the entries' own slots (a zero
// difference enters as 1), the powers and derivative powers of the targets, the three tile products (terms cut across four
// waves, one unreduced accumulator and one reduction per wave, the four parts added mod p) and the finish rule -- against
// Horner's rule on the polynomial that Berlekamp-Welch finds on the sub-row of the columns that are not erased.
// Stand-alone: shamir_wide_evaluate <prime in hex>...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pvw_wide.h"

using namespace pvw;

struct W4 {
  u64 v[4];
};
static const u32 UNDECODABLE = 0xFFFFFFFFu;

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
static W4 add(W4 a, const W4& b, const WideMont& m) {
  wide_add_p(a.v, b.v, m);
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

struct Report {
  W4 out;
  u32 nerr;
  std::vector<u32> wrong;
  bool operator==(const Report& o) const { return !memcmp(out.v, o.out.v, 32) && nerr == o.nerr && wrong == o.wrong; }
};

// the kernels' decode of one row: x [count] times R, y [count] any words, er [count] the row's mask; t the degree
// psi_out [r + 1] (reversed, times R), M_out [count] (times R) and u_out [count] (times R) are what the evaluation reads
static Report kernel_decode(const std::vector<W4>& x, const std::vector<W4>& yw, const std::vector<bool>& er, u32 t, const WideMont& m,
                            std::vector<W4>& psi_out, std::vector<W4>& M_out, std::vector<W4>& u_out) {
  const u32 count = (u32)x.size(), r = count - t - 1;
  const W4 zero = {{0, 0, 0, 0}};
  Report rep{zero, UNDECODABLE, {}};
  // u_c = (prod_{i != c}(x_c - x_i))^-1, P = prod(-x_i), lambda_c = u_c P / (-x_c), all times R
  std::vector<W4> u(count), lam(count), y(count);
  W4 Pn = one(m);
  for (u32 c = 0; c < count; ++c) {
    W4 pr = one(m);
    for (u32 i = 0; i < count; ++i)
      if (i != c) pr = mul(pr, sub(x[c], x[i], m), m);
    u[c] = inv(pr, m);
    Pn = mul(Pn, sub(zero, x[c], m), m);
  }
  for (u32 c = 0; c < count; ++c) lam[c] = mul(mul(u[c], Pn, m), inv(sub(zero, x[c], m), m), m);
  u_out = u;
  psi_out.assign(r + 1, zero);
  M_out.assign(count, zero);
  for (u32 c = 0; c < count; ++c) {
    y[c] = zero;
    if (!er[c]) wide_reduce_p(yw[c].v, m, y[c].v);             // an erased element is not loaded: it is staged as 0
  }
  // Synd[j] = sum_c y_c (u_c x_c^j R), reduced once: plain
  std::vector<W4> S(r);
  {
    std::vector<W4> v = u;
    for (u32 j = 0; j < r; ++j) {
      u32 acc[16];
      wide_acc_zero(acc);
      for (u32 c = 0; c < count; ++c) {
        u32 P[16];
        wide_mul_full(y[c].v, v[c].v, P);
        wide_acc_add(acc, P, m);
        v[c] = mul(v[c], x[c], m);
      }
      wide_redc(acc, m, S[j].v);
    }
  }
  u32 eps = 0;
  for (u32 c = 0; c < count; ++c) eps += er[c];
  if (eps > r) return rep;
  // Gamma times R, one factor per erased column in the order of the columns, each walked downwards in blocks of 64
  std::vector<W4> G(eps + 1, zero);
  G[0] = one(m);
  u32 g = 0;
  for (u32 c = 0; c < count; ++c) {
    if (!er[c]) continue;
    for (u32 k = (g + 1) / 64 + 1; k-- > 0;) {
      W4 cur[64], prev[64];
      for (u32 l = 0; l < 64; ++l) {                 // every lane reads before any lane writes
        const u32 i = k * 64 + l;
        cur[l] = i <= g ? G[i] : zero;
        prev[l] = i <= g + 1 && i >= 1 ? G[i - 1] : zero;
      }
      for (u32 l = 0; l < 64; ++l) {
        const u32 i = k * 64 + l;
        if (i <= g + 1) G[i] = sub(cur[l], mul(x[c], prev[l], m), m);
      }
    }
    ++g;
  }
  // the Forney syndromes over S[eps ..], blocks downwards; each one unreduced accumulator and one reduction
  const u32 nT = r - eps, E = nT / 2;
  if (eps)
    for (u32 k = (nT + 63) / 64; k-- > 0;) {
      W4 val[64];
      for (u32 l = 0; l < 64; ++l) {
        const u32 idx = k * 64 + l, n = eps + idx;
        if (idx >= nT) continue;
        u32 acc[16];
        wide_acc_zero(acc);
        for (u32 i = 0; i <= eps; ++i) {
          u32 P[16];
          wide_mul_full(G[i].v, S[n - i].v, P);
          wide_acc_add(acc, P, m);
        }
        wide_redc(acc, m, val[l].v);
      }
      for (u32 l = 0; l < 64; ++l)
        if (k * 64 + l < nT) S[eps + k * 64 + l] = val[l];
    }
  const W4* T = S.data() + eps;
  // Berlekamp-Massey on T: C, B, b times R; d plain, then times R for the update
  std::vector<W4> C(E + 1, zero), B(E + 1, zero);
  C[0] = B[0] = one(m);
  u32 L = 0, mm = 1;
  W4 bsc = one(m);
  for (u32 n = 0; n < nT; ++n) {
    u32 acc[64][16];
    for (u32 l = 0; l < 64; ++l) wide_acc_zero(acc[l]);
    for (u32 i = 0; i <= L; ++i) {
      u32 P[16];
      wide_mul_full(C[i].v, T[n - i].v, P);
      wide_acc_add(acc[i % 64], P, m);
    }
    W4 d = zero;
    for (u32 l = 0; l < 64; ++l) {
      W4 part;
      wide_redc(acc[l], m, part.v);
      d = add(d, part, m);
    }
    if (is0(d)) { ++mm; continue; }
    const bool grow = 2 * L <= n;
    const u32 Ln = grow ? n + 1 - L : L;
    if (Ln > E) return rep;
    wide_mont_in(d.v, m, d.v);
    for (u32 k = Ln / 64 + 1; k-- > 0;) {
      W4 c[64], bb[64];
      for (u32 l = 0; l < 64; ++l) {
        const u32 i = k * 64 + l;
        c[l] = i <= Ln ? C[i] : zero;
        bb[l] = i <= Ln && i >= mm ? B[i - mm] : zero;
      }
      for (u32 l = 0; l < 64; ++l) {
        const u32 i = k * 64 + l;
        if (i > Ln) continue;
        C[i] = sub(mul(bsc, c[l], m), mul(d, bb[l], m), m);
        if (grow) B[i] = c[l];
      }
    }
    if (grow) { L = Ln; bsc = d; mm = 1; } else { ++mm; }
  }
  // psi[k] = Psi_{L_s - k} R for k <= L_s, 0 up to r; Psi_j = sum_i Lambda_i Gamma_{j-i}
  const u32 Ls = eps + L;
  std::vector<W4> psi(r + 1, zero);
  for (u32 k = 0; k <= Ls; ++k) {
    const u32 j = Ls - k;
    u32 acc[16];
    wide_acc_zero(acc);
    for (u32 i = j > eps ? j - eps : 0; i <= L && i <= j; ++i) {
      u32 P[16];
      wide_mul_full(C[i].v, G[j - i].v, P);
      wide_acc_add(acc, P, m);
    }
    wide_redc(acc, m, psi[k].v);
  }
  // M[c] = sum_{k <= r} psi[k] (x_c^k R): times R
  std::vector<W4> M(count);
  u32 nz = 0;
  for (u32 c = 0; c < count; ++c) {
    u32 acc[16];
    wide_acc_zero(acc);
    W4 pw = one(m);
    for (u32 k = 0; k <= r; ++k) {
      W4 lk;
      wide_reduce_p(psi[k].v, m, lk.v);
      u32 P[16];
      wide_mul_full(lk.v, pw.v, P);
      wide_acc_add(acc, P, m);
      pw = mul(pw, x[c], m);
    }
    wide_redc(acc, m, M[c].v);
    nz += is0(M[c]);
  }
  psi_out = psi;
  M_out = M;
  if (nz != Ls) return rep;
  u32 acc[16];
  wide_acc_zero(acc);
  for (u32 c = 0; c < count; ++c) {
    if (is0(M[c])) {
      if (!er[c]) rep.wrong.push_back(c);
      continue;
    }
    W4 yc;
    wide_reduce_p(yw[c].v, m, yc.v);                 // the finish kernel reads the share itself
    const W4 w = mul(lam[c], M[c], m);
    u32 P[16];
    wide_mul_full(yc.v, w.v, P);
    wide_acc_add(acc, P, m);
  }
  W4 v;
  wide_redc(acc, m, v.v);
  rep.out = mul(v, inv(psi[0], m), m);
  rep.nerr = Ls - eps;
  return rep;
}

// Berlekamp-Welch: N of degree <= t + E and monic W of degree E with N(x_c) = y_c W(x_c); N / W is compared with the row
// F [t + 1]: the coefficients of N / W, times R, for a decodable row
static Report welch(const std::vector<W4>& x, const std::vector<W4>& yw, u32 t, const WideMont& m, std::vector<W4>& F) {
  const size_t count = x.size(), E = (count - t - 1) / 2, nq = t + E + 1, nu = nq + E, ld = nu + 1;
  const W4 zero = {{0, 0, 0, 0}};
  std::vector<W4> y(count), A(count * ld, zero), sol(nu, zero), Wp(E + 1), N(nq);
  for (size_t c = 0; c < count; ++c) wide_mont_in(yw[c].v, m, y[c].v);
  for (size_t c = 0; c < count; ++c) {
    W4 pw = one(m);
    for (size_t j = 0; j < nq; ++j) {
      A[c * ld + j] = pw;
      if (j < E) A[c * ld + nq + j] = sub(zero, mul(y[c], pw, m), m);
      if (j == E) A[c * ld + nu] = mul(y[c], pw, m);
      pw = mul(pw, x[c], m);
    }
  }
  std::vector<size_t> pivot;
  size_t rank = 0;
  for (size_t col = 0; col < nu && rank < count; ++col) {
    size_t pr = rank;
    while (pr < count && is0(A[pr * ld + col])) ++pr;
    if (pr == count) continue;
    for (size_t j = 0; j < ld && pr != rank; ++j) std::swap(A[pr * ld + j], A[rank * ld + j]);
    const W4 iv = inv(A[rank * ld + col], m);
    for (size_t j = col; j <= nu; ++j) A[rank * ld + j] = mul(A[rank * ld + j], iv, m);
    for (size_t i = 0; i < count; ++i) {
      const W4 f = A[i * ld + col];
      if (i == rank || is0(f)) continue;
      for (size_t j = col; j <= nu; ++j) A[i * ld + j] = sub(A[i * ld + j], mul(f, A[rank * ld + j], m), m);
    }
    pivot.push_back(col);
    ++rank;
  }
  Report rep{zero, UNDECODABLE, {}};
  for (size_t i = rank; i < count; ++i)
    if (!is0(A[i * ld + nu])) return rep;
  for (size_t i = 0; i < rank; ++i) sol[pivot[i]] = A[i * ld + nu];
  for (size_t j = 0; j < nq; ++j) N[j] = sol[j];
  for (size_t k = 0; k < E; ++k) Wp[k] = sol[nq + k];
  Wp[E] = one(m);
  for (size_t i = nq; i-- > E;) {
    const W4 f = N[i];
    for (size_t k = 0; k < E; ++k) N[i - E + k] = sub(N[i - E + k], mul(f, Wp[k], m), m);
  }
  for (size_t k = 0; k < E; ++k)
    if (!is0(N[k])) return rep;
  std::vector<u32> wrong;
  for (size_t c = 0; c < count; ++c) {
    W4 v = N[E + t];
    for (size_t j = t; j-- > 0;) v = add(mul(v, x[c], m), N[E + j], m);
    if (memcmp(v.v, y[c].v, 32) != 0) wrong.push_back((u32)c);
  }
  if (wrong.size() > E) return rep;
  wide_mont_out(N[E].v, m, rep.out.v);
  F.assign(N.begin() + E, N.begin() + E + t + 1);
  rep.nerr = (u32)wrong.size();
  rep.wrong = wrong;
  return rep;
}

// the contract: Berlekamp-Welch with the same t on the sub-row of the columns that are not erased, the wrong columns mapped back
static Report contract(const std::vector<W4>& x, const std::vector<W4>& y, const std::vector<bool>& er, u32 t, const WideMont& m,
                       std::vector<W4>& F) {
  std::vector<W4> xs, ys;
  std::vector<u32> cols;
  for (u32 c = 0; c < x.size(); ++c)
    if (!er[c]) {
      xs.push_back(x[c]);
      ys.push_back(y[c]);
      cols.push_back(c);
    }
  Report rep{{{0, 0, 0, 0}}, UNDECODABLE, {}};
  if (xs.size() < (size_t)t + 1) return rep;
  rep = welch(xs, ys, t, m, F);
  for (u32& c : rep.wrong) c = cols[c];
  return rep;
}

// the tile product's sum for one output: terms cut across four waves (wave w owns [w Q, w Q + Q)), a[j] any words read below p
// and staged, b[j] times R; each wave one unreduced accumulator and one reduction, the four parts added mod p
static W4 tile_sum(const std::vector<W4>& a, const std::vector<W4>& b, const WideMont& m) {
  const u32 nt = (u32)a.size(), Q = (nt + 3) / 4;
  W4 v = {{0, 0, 0, 0}};
  for (u32 w = 0; w < 4; ++w) {
    u32 acc[16];
    wide_acc_zero(acc);
    for (u32 j = w * Q; j < nt && j < w * Q + Q; ++j) {
      W4 aj;
      wide_reduce_p(a[j].v, m, aj.v);
      u32 P[16];
      wide_mul_full(aj.v, b[j].v, P);
      wide_acc_add(acc, P, m);
    }
    W4 part;
    wide_redc(acc, m, part.v);
    v = w ? add(v, part, m) : part;
  }
  return v;
}

static const u32 NO_COLUMN = 0xFFFFFFFFu, BATCH = 32;

// the kernels' evaluation of one row at the targets xt (times R): values [T] plain; decodable: what the decode's finish reported
static std::vector<W4> kernel_evaluate(const std::vector<W4>& x, const std::vector<W4>& u, const std::vector<W4>& yw,
                                       const std::vector<W4>& psi, const std::vector<W4>& M, bool decodable, const std::vector<W4>& xt,
                                       const WideMont& m) {
  const u32 count = (u32)x.size(), T = (u32)xt.size(), nk = (u32)psi.size();
  const W4 zero = {{0, 0, 0, 0}};
  // YM[c] = REDC(y_c (M_c R)), the share's own words; where M is 0 the share is not read
  std::vector<W4> YM(count, zero);
  for (u32 c = 0; c < count; ++c)
    if (!is0(M[c])) wide_mont_mul(yw[c].v, M[c].v, m, YM[c].v);
  // scale_j and the coinciding column: lane l takes the columns l, l + 64, ...; the lanes meet by xor steps 32, 16, .. 1
  std::vector<W4> scale(T);
  std::vector<u32> coin(T);
  for (u32 j = 0; j < T; ++j) {
    W4 prod[64];
    u32 hit[64];
    for (u32 l = 0; l < 64; ++l) {
      prod[l] = one(m);
      hit[l] = NO_COLUMN;
      for (u32 i = l; i < count; i += 64) {
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
  // C[i][j] = u_i / (x*_j - x_i): BATCH differences per inversion, the running products in the entries' own slots
  std::vector<W4> C((size_t)count * T);
  for (u32 i0 = 0; i0 < count; i0 += BATCH)
    for (u32 j = 0; j < T; ++j) {
      const u32 cnt = count - i0 < BATCH ? count - i0 : BATCH;
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
  // Xt[k][j] = x*^k and Xd[k][j] = k x*^(k-1), times R; k R by additions of R
  std::vector<W4> Xt((size_t)nk * T), Xd((size_t)nk * T);
  for (u32 j = 0; j < T; ++j) {
    W4 pw = one(m), dv = one(m), kr = zero;
    for (u32 k = 0; k < nk; ++k) {
      Xt[(size_t)k * T + j] = pw;
      pw = mul(pw, xt[j], m);
      W4 o = zero;
      if (k) {
        o = mul(kr, dv, m);
        dv = mul(dv, xt[j], m);
      }
      Xd[(size_t)k * T + j] = o;
      kr = add(kr, one(m), m);
    }
  }
  std::vector<W4> values(T, zero);
  for (u32 j = 0; j < T; ++j) {
    std::vector<W4> cj(count), tj(nk), dj(nk);
    for (u32 i = 0; i < count; ++i) cj[i] = C[(size_t)i * T + j];
    for (u32 k = 0; k < nk; ++k) tj[k] = Xt[(size_t)k * T + j], dj[k] = Xd[(size_t)k * T + j];
    const W4 raw = tile_sum(YM, cj, m), psiT = tile_sum(psi, tj, m), psiD = tile_sum(psi, dj, m);
    if (!decodable) continue;
    const u32 c = coin[j];
    if (c != NO_COLUMN && !is0(M[c])) {
      wide_reduce_p(yw[c].v, m, values[j].v);
    } else {
      const W4 den = c != NO_COLUMN ? psiD : psiT;
      if (is0(den)) {
        printf("a zero denominator in a decodable row\n");
        exit(1);
      }
      values[j] = mul(mul(raw, scale[j], m), inv(den, m), m);
    }
  }
  return values;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  long decodable = 0, undecodable = 0, beyond = 0, checked = 0;
  for (int a = 1; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p) || !(p[0] & 1)) return 2;
    const WideMont m = make_wide_mont(p);
    const bool above_2_64 = p[2] || p[3] || p[1] > 1 || (p[1] == 1 && p[0] != 0);
    rng_state = 0xE7A5E500 + (u64)a;
    // the shapes: t 0..3 x r 0..7, and every (eps, nu) with eps <= r + 1 and nu <= E_s + 1; for the first and the last prime one
    // row with r = 200, eps = 70 and E_s = 65 errors: Gamma, the Forney pass and the locator each span more than one block of 64
    // the points come from 1 .. pool: 60000 of them, or every point of the field where p has fewer; a tiny p keeps the shapes
    // whose points it can tell apart (count <= pool)
    const u64 pool = (p[1] | p[2] | p[3]) || p[0] > 60000 ? 60000 : p[0] - 1;
    struct Shape { u32 t, r, eps, nu; };
    std::vector<Shape> shapes;
    for (u32 t = 0; t < 4; ++t)
      for (u32 r = 0; r < 8 && t + 1 + r <= pool; ++r)
        for (u32 eps = 0; eps <= r + 1; ++eps) {
          const u32 Es = eps <= r ? (r - eps) / 2 : 0;
          for (u32 nu = 0; nu <= Es + 1 && eps + nu <= t + 1 + r; ++nu) shapes.push_back({t, r, eps, nu});
        }
    if ((a == 1 || a == argc - 1) && pool >= 203) shapes.push_back({2, 200, 70, 65});
    for (size_t i = 0; i < shapes.size(); ++i) {
      const u32 t = shapes[i].t, r = shapes[i].r, eps = shapes[i].eps, nu = shapes[i].nu, count = t + 1 + r;
      std::vector<W4> x(count), y(count), co(t + 1);
      std::vector<u64> pts;
      while (pts.size() < count) {
        u64 v = 1 + rnd64() % pool;                            // below the prime
        if (pts.empty() && above_2_64) v = 0;                    // stands for the point 2^64 (index 2^64 - 1)
        bool dup = false;
        for (u64 q : pts) dup |= q == v;
        if (!dup) pts.push_back(v);
      }
      for (u32 c = 0; c < count; ++c) {
        const u64 xw[4] = {pts[c], pts[c] == 0 ? (u64)1 : (u64)0, 0, 0};
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
      // eps + nu distinct columns: the first eps erased and filled with junk, the others overwritten
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
          y[c].v[rnd64() % 4] ^= (u64)1 << (rnd64() % 64);     // any words: read mod p by both sides
        }
      }
      std::vector<W4> psi, M, u, F;
      const Report got = kernel_decode(x, y, er, t, m, psi, M, u), want = contract(x, y, er, t, m, F);
      // the targets: every column's point (a zero difference at that column's position of its batch; right, wrong and erased
      // columns), three points that are no column's, and the first column once more
      std::vector<W4> xt = x;
      for (u32 k = 0; k < 3; ++k) {
        // above every column's point and below the prime; where p has no such point, any point of the field
        const u64 xw[4] = {pool == 60000 && ((p[1] | p[2] | p[3]) || p[0] > 65001) ? 60001 + rnd64() % 5000 : 1 + rnd64() % pool, 0, 0, 0};
        W4 v;
        wide_mont_in(xw, m, v.v);
        xt.push_back(v);
      }
      xt.push_back(x[0]);
      const std::vector<W4> values = kernel_evaluate(x, u, y, psi, M, got.nerr != UNDECODABLE, xt, m);
      for (size_t j = 0; j < xt.size(); ++j) {
        W4 v = {{0, 0, 0, 0}};
        if (want.nerr != UNDECODABLE) {
          v = F[t];
          for (u32 k = t; k-- > 0;) v = add(mul(v, xt[j], m), F[k], m);
          wide_mont_out(v.v, m, v.v);
        }
        if (memcmp(v.v, values[j].v, 32) != 0) {
          printf("VALUE MISMATCH prime %s shape %zu (t %u r %u eps %u nu %u) target %zu of %zu\n", argv[a], i, t, r, eps, nu, j, xt.size());
          return 1;
        }
        ++checked;
      }
      if (!(got == want)) {
        printf("MISMATCH prime %s shape %zu (t %u r %u eps %u nu %u): nerr %u / %u\n", argv[a], i, t, r, eps, nu, got.nerr, want.nerr);
        return 1;
      }
      for (u32 c : got.wrong)
        if (er[c]) {
          printf("an erased column is reported: prime %s shape %zu\n", argv[a], i);
          return 1;
        }
      if (eps <= r && nu == 0 && want.nerr != 0) {
        printf("a consistent sub-row is not decoded: prime %s shape %zu\n", argv[a], i);
        return 1;
      }
      if (eps > r && want.nerr != UNDECODABLE) return 1;
      if (eps > r || nu > (r - eps) / 2) ++beyond;
      (want.nerr == UNDECODABLE ? undecodable : decodable)++;
    }
  }
  if (!decodable || !undecodable || !beyond) return 1;
  printf("SHAMIR_WIDE_EVALUATE_OK %ld decodable %ld undecodable %ld beyond the bound, %ld values\n", decodable, undecodable, beyond, checked);
  return 0;
}

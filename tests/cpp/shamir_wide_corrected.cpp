// The decode of corrected reconstruction over a prime below 2^256 (pvw_rs_amd/csrc/pvw_shamir.hip), restated
// sequentially in the kernels' update order and forms over pvw_wide.h's own product, accumulator and reduction -- syndromes,
// the inversion-free Berlekamp-Massey recurrence with 64 lane accumulators and the downward walk in blocks of 64, the locator at
// every point, the zero count and the finish formula -- against Berlekamp-Welch by Gaussian elimination, whose last step is the
// contract itself.  Stand-alone: shamir_wide_corrected <rows per prime> <prime in hex>...
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

// the kernels' decode of one row: x [count] times R, y [count] any words; t the degree
static Report kernel_decode(const std::vector<W4>& x, const std::vector<W4>& yw, u32 t, const WideMont& m) {
  const u32 count = (u32)x.size(), r = count - t - 1, E = r / 2;
  const W4 zero = {{0, 0, 0, 0}};
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
  for (u32 c = 0; c < count; ++c) wide_reduce_p(yw[c].v, m, y[c].v);
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
  // Berlekamp-Massey: C, B, b times R; d plain, then times R for the update
  std::vector<W4> C(E + 1, zero), B(E + 1, zero);
  C[0] = B[0] = one(m);
  u32 L = 0, mm = 1;
  W4 bsc = one(m);
  bool ok = true;
  for (u32 n = 0; n < r && ok; ++n) {
    u32 acc[64][16];
    for (u32 l = 0; l < 64; ++l) wide_acc_zero(acc[l]);
    for (u32 i = 0; i <= L; ++i) {
      u32 P[16];
      wide_mul_full(C[i].v, S[n - i].v, P);
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
    if (Ln > E) { ok = false; break; }
    wide_mont_in(d.v, m, d.v);
    for (u32 k = Ln / 64 + 1; k-- > 0;) {
      W4 c[64], bb[64];
      for (u32 l = 0; l < 64; ++l) {                 // every lane reads before any lane writes
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
  Report rep{zero, UNDECODABLE, {}};
  if (!ok) return rep;
  // Lambda[k] = C[L - k]; M[c] = sum_k Lambda[k] (x_c^k R): times R
  std::vector<W4> M(count);
  u32 nz = 0;
  for (u32 c = 0; c < count; ++c) {
    u32 acc[16];
    wide_acc_zero(acc);
    W4 pw = one(m);
    for (u32 k = 0; k <= E; ++k) {
      const W4 src = k <= L ? C[L - k] : zero;
      W4 lk;
      wide_reduce_p(src.v, m, lk.v);
      u32 P[16];
      wide_mul_full(lk.v, pw.v, P);
      wide_acc_add(acc, P, m);
      pw = mul(pw, x[c], m);
    }
    wide_redc(acc, m, M[c].v);
    nz += is0(M[c]);
  }
  if (nz != L) return rep;
  u32 acc[16];
  wide_acc_zero(acc);
  for (u32 c = 0; c < count; ++c) {
    if (is0(M[c])) { rep.wrong.push_back(c); continue; }
    const W4 w = mul(lam[c], M[c], m);
    u32 P[16];
    wide_mul_full(y[c].v, w.v, P);
    wide_acc_add(acc, P, m);
  }
  W4 v;
  wide_redc(acc, m, v.v);
  rep.out = mul(v, inv(C[L], m), m);
  rep.nerr = L;
  return rep;
}

// Berlekamp-Welch: N of degree <= t + E and monic W of degree E with N(x_c) = y_c W(x_c); N / W is compared with the row
static Report welch(const std::vector<W4>& x, const std::vector<W4>& yw, u32 t, const WideMont& m) {
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
  rep.nerr = (u32)wrong.size();
  rep.wrong = wrong;
  return rep;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long cases = atol(argv[1]);
  long decodable = 0, undecodable = 0;
  for (int a = 2; a < argc; ++a) {
    u64 p[4];
    if (!parse_hex(argv[a], p) || !(p[0] & 1)) return 2;
    const WideMont m = make_wide_mont(p);
    const bool above_2_64 = p[2] || p[3] || p[1] > 1 || (p[1] == 1 && p[0] != 0);
    rng_state = 0xDEC0DE00 + (u64)a;
    // the points come from 1 .. pool: 60000 of them, or every point of the field where p has fewer; a tiny p cuts t and r
    // down to the shapes whose points it can tell apart (count <= pool)
    const u64 pool = (p[1] | p[2] | p[3]) || p[0] > 60000 ? 60000 : p[0] - 1;
    for (long i = 0; i < cases; ++i) {
      // the shapes in turn: t 0..6, r 0..9; for the first and the last prime one row with E = 66 errors, whose locator spans more
      // than one block of 64 coefficients (r = 132)
      const bool big = i == cases - 1 && (a == 2 || a == argc - 1) && pool >= 140;
      const u32 t = (u32)((u64)(i % 7) % pool), rmax = (u32)(pool - t < 10 ? pool - t : 10);
      const u32 r = big ? 132 : (u32)((i / 7 + i) % rmax), count = t + 1 + r, E = r / 2;
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
      const u32 mode = big ? 2 : (u32)(i % 5);                          // 0: consistent; 1: one error; 2: E; 3: E + 1; 4: any words
      const u32 nbad = mode == 0 ? 0 : mode == 1 ? (count ? 1 : 0) : mode == 2 ? E : E + 1;
      for (u32 c = 0; c < count; ++c) {
        W4 v = co[t];
        for (u32 j = t; j-- > 0;) v = add(mul(v, x[c], m), co[j], m);
        wide_mont_out(v.v, m, y[c].v);
      }
      for (u32 k = 0; k < nbad && mode != 4; ++k) {
        const u32 c = (u32)((rnd64() % count + k) % count);
        y[c].v[rnd64() % 4] ^= (u64)1 << (rnd64() % 64);       // any words: read mod p by both sides
      }
      if (mode == 4)
        for (u32 c = 0; c < count; ++c)
          for (int k = 0; k < 4; ++k) y[c].v[k] = c == 0 ? ~(u64)0 : rnd64();
      const Report got = kernel_decode(x, y, t, m), want = welch(x, y, t, m);
      if (!(got == want)) {
        printf("MISMATCH prime %s case %ld (t %u r %u mode %u): nerr %u / %u\n", argv[a], i, t, r, mode, got.nerr, want.nerr);
        return 1;
      }
      if (mode == 0 && want.nerr != 0) {
        printf("a consistent row is not decoded: prime %s case %ld\n", argv[a], i);
        return 1;
      }
      (want.nerr == UNDECODABLE ? undecodable : decodable)++;
    }
  }
  if (!decodable || !undecodable) return 1;
  printf("SHAMIR_WIDE_CORRECTED_OK %ld decodable %ld undecodable\n", decodable, undecodable);
  return 0;
}

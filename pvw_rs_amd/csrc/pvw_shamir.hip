// pvw_shamir.hip -- Shamir shares on gfx950: shares[d][i] = f_d(i + 1) mod p with
// f_d(x) = s_d + a_{d,1} x + ... + a_{d,t} x^t, for every dealer d and every party i of the context's range.
// The reference has no sharing code (its examples fill the share matrix with arbitrary numbers): the contract is this
// library's own and pvw_shamir_shares_host (pvw_capi.hip) is its plain restatement.
//
// Shape (shamir_eval_kernel).  A lane owns one party (x = i + 1) and SH_DG dealers; the four waves of a workgroup own the same
// 64 parties and dealers and a quarter of the terms each.  Term e of the unpacked kernel is j = e + 1: a wave starts from
// x^(j0) by square-and-multiply and then keeps pw = x^j up to date with ONE full modular multiply per term, shared by its
// dealers; a_{d,j} pw goes into one lazy accumulator per dealer (pvw_arith.h: 4 x v_mad_u64_u32 into independent sums, reduced
// once at the end).  The four partial sums meet in LDS, as mac_rows sums its waves, and the secret is added there.
// Coefficients are uniform across a wave: each chunk of SH_JC terms per wave is staged in LDS by the whole workgroup and
// read back as broadcasts ([wave][term][dealer], so one term's SH_DG coefficients are one 32-byte read at the same address
// in every lane).  Drawn coefficients are MADE in that staging phase -- one lane per coefficient, one ChaCha8 block per
// try, its words statically indexed -- so nothing but the shares is ever written to memory; every workgroup of a dealer
// group repeats the draw for its 64 parties (about a quarter of the multiply-add work at 64 parties per workgroup).
//
// PACKED: K secrets per dealer at the points 0, -1, ..., -(K-1) (Franklin-Yung),
//   f_d(x) = sum_{j<K} s_{d,j} L_j(x) + Z(x) (a_{d,1} + a_{d,2} x + ... + a_{d,t} x^(t-1)),  Z(x) = x (x+1) ... (x+K-1).
// The term axis becomes e = 0 .. K + t - 1.  e < K is secret term e: coefficient s_{d,e}, staged like any other, and weight
// Lw[e][party], LOADED, four in flight ahead of their multiply-adds as in shamir_tile_product.  e >= K is random term
// j = e - K + 1: weight Z(x) x^(j-1) = zt(x) x^j, the running power started from x^(j0) zt(x) at the wave's first random term.
// Nothing is added at the meet.  With K = 1, Lw = zt = 1 and the sum is the unpacked one, term for term -- at one loaded
// weight per secret term and one more multiply per lane, which is why the unpacked entry points keep an instantiation of
// their own (K = 0 loaded terms, no Lw, no zt) rather than run the packed one at K = 1.
#include <hip/hip_runtime.h>

#include "pvw_arith.h"
#include "pvw_chacha.h"
#include "pvw_kernels.h"

namespace pvw {

#define SH_DG 4      // dealers per lane
#define SH_JC 64     // terms per wave and staging chunk
#define SH_WAVES 4

// a_{d,j}: the first accepted draw of the stream (key of dealer d, id (DOM_SHAMIR << 32) | j), by the rule of
// sample_residues_poly: next_u64() >> clz(p), accepted when < p.  The stream makes this one value only, so the draws of
// a block are tried in order with static word indices.
PVW_HD u64 shamir_draw(const ChaChaKey& key, u32 j, u64 p, u32 sh) {
  ChaChaRng g;
  g.init(key, DOM_SHAMIR, j);
  for (;;) {
    g.refill();
    u64 val = 0;
    bool got = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u64 v = ((u64)g.buf[2 * i] | ((u64)g.buf[2 * i + 1] << 32)) >> sh;
      if (!got && v < p) { val = v; got = true; }
    }
    if (got) return val;
  }
}

// b^e; the exponent keeps its width: a u32 is walked in 32-bit registers, and a^(p - 2) (invmod_dev) needs 64
template <class E>
__device__ __forceinline__ u64 powmod_dev(u64 b, E e, const Mod& m) {
  u64 r = 1;
  while (e) {
    if (e & 1) r = mulmod(r, b, m);
    b = mulmod(b, b, m);
    e >>= 1;
  }
  return r;
}
__device__ __forceinline__ u64 invmod_dev(u64 a, const Mod& m) { return powmod_dev(a, m.q - 2, m); }   // Fermat

// The loaded multiply-adds of the frame: acc[g] += a[jj][g] * wp[jj * stride] for the terms jj < cnt of a wave's chunk `a`, four
// weights in flight ahead of their multiply-adds, then the tail.  A lane that is not live loads nothing and adds 0.
__device__ __forceinline__ void shamir_mac_loaded(Acc (&acc)[SH_DG], const u64 (*a)[SH_DG], const u64* wp, size_t stride, u32 cnt,
                                                  bool live) {
  u32 jj = 0;
  for (; jj + 4 <= cnt; jj += 4) {
    u64 w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = live ? wp[(size_t)u * stride] : 0;
    wp += (size_t)4 * stride;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      u64 v[SH_DG];
#pragma unroll
      for (int g = 0; g < SH_DG; ++g) v[g] = a[jj + u][g];
#pragma unroll
      for (int g = 0; g < SH_DG; ++g) acc_mac_dev(acc[g], v[g], w[u]);
    }
  }
  for (; jj < cnt; ++jj) {
    const u64 w = live ? *wp : 0;
    wp += stride;
    u64 v[SH_DG];
#pragma unroll
    for (int g = 0; g < SH_DG; ++g) v[g] = a[jj][g];
#pragma unroll
    for (int g = 0; g < SH_DG; ++g) acc_mac_dev(acc[g], v[g], w);
  }
}

// how many terms chunk c holds of the wave whose range is [w0, w0 + Q) cut off at nt; the chunk's first is w0 + c * SH_JC
__device__ __forceinline__ u32 shamir_chunk_terms(u32 w0, u32 Q, u32 c, u32 nt) {
  const u32 base = c * SH_JC;
  u32 cnt = 0;
  if (base < Q && w0 + base < nt) {
    cnt = Q - base < SH_JC ? Q - base : SH_JC;
    const u32 left = nt - (w0 + base);
    cnt = left < cnt ? left : cnt;
  }
  return cnt;
}

// The four waves' partial sums meet in LDS: thread (wave = g, lane) comes back with v plus accumulator g of every wave, below
// p; a thread that is not live with v.  m by value (shamir_tile_product).  part is the caller's, declared BEHIND its staging
// array: declared here it lands in front of it, and shamir_interp_kernel then measured 2 % slower at 64 secrets
// (profiles/r12_shamir_deal_fold.txt).
__device__ __forceinline__ u64 shamir_meet(Acc (&acc)[SH_DG], u64 (&part)[SH_WAVES][SH_DG][64], u64 v, bool live, const Mod m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int g = 0; g < SH_DG; ++g) part[wave][g][lane] = acc_reduce(acc[g], m);
  __syncthreads();
  if (live) {
#pragma unroll
    for (int w = 0; w < SH_WAVES; ++w) v = addmod(v, part[w][wave][lane], m.q);   // SH_WAVES == SH_DG
  }
  return v;
}
static_assert(SH_WAVES == SH_DG, "the last phase maps one wave to one dealer of the group");

// grid: x = blocks of 64 parties of [party_lo, party_hi), y = groups of SH_DG dealers; 256 threads.
template <bool PACKED>
__global__ __launch_bounds__(256) void shamir_eval_kernel(ShamirBatch b) {
  __shared__ u64 coef[SH_WAVES][SH_JC][SH_DG];     // 8 KiB: the chunk's coefficients, below p
  __shared__ u64 part[SH_WAVES][SH_DG][64];        // 8 KiB: the waves' partial sums, below p
  __shared__ u32 keyw[SH_DG][8];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Mod m = b.m;
  const u32 t = b.degree, K = PACKED ? b.pack : 0, nt = K + t;
  const u32 d0 = blockIdx.y * SH_DG;
  const u32 col = blockIdx.x * 64 + lane;
  const u32 cols = b.party_hi - b.party_lo;
  const u32 party = b.party_lo + col;
  const bool live = col < cols;
  const bool drawn = b.coeffs == nullptr && t != 0;
  const u32 sh = (u32)__clzll((long long)m.q);
  if (drawn && tid < SH_DG && d0 + tid < b.nd) {
    ChaChaKey k;
    if (b.rnd) k = call_seed(b.rnd->seed, b.rnd->counter + b.rnd_off + d0 + tid);   // derived when the kernel runs
    else k = b.key[d0 + tid];
#pragma unroll
    for (int i = 0; i < 8; ++i) keyw[tid][i] = k.w[i];
  }
  // wave w owns terms e = w * Q + [0, Q), cut off at nt; every wave walks the same number of chunks (barriers)
  const u32 Q = (nt + SH_WAVES - 1) / SH_WAVES;
  const u32 ew0 = wave * Q;
  const u32 ew1 = ew0 + Q < nt ? ew0 + Q : nt;     // the end of the wave's range (ew1 <= ew0: none)
  const u32 nchunks = (Q + SH_JC - 1) / SH_JC;
  const u64 x = live ? (u64)party + 1 : 1;         // x <= n < p
  // the wave's first random term e, j = e - K + 1, and its weight x^j (packed: zt(x) x^j)
  const u32 er0 = ew0 > K ? ew0 : K;
  u64 pw = 0;
  if (er0 < ew1) {
    pw = powmod_dev(x, er0 - K + 1, m);
    if (PACKED) pw = mulmod(pw, live ? b.zt[col] : 0, m);
  }
  Acc acc[SH_DG];
#pragma unroll
  for (int g = 0; g < SH_DG; ++g) acc_zero(acc[g]);
  __syncthreads();
  for (u32 c = 0; c < nchunks; ++c) {
    // ---- staging: entry e = (wave, term, dealer) of the chunk, one per lane and trip ----
    for (u32 e = tid; e < SH_WAVES * SH_JC * SH_DG; e += 256) {
      const u32 ew = e / (SH_JC * SH_DG), ej = (e / SH_DG) % SH_JC, eg = e % SH_DG;
      const u32 off = c * SH_JC + ej;              // within the wave's range
      const u32 te = ew * Q + off;                 // the term
      u64 a = 0;
      if (off < Q && te < nt && d0 + eg < b.nd) {
        if (te < K) {
          a = reduce_word(b.secrets[(size_t)(d0 + eg) * K + te], m);
        } else if (drawn) {
          ChaChaKey k;
#pragma unroll
          for (int i = 0; i < 8; ++i) k.w[i] = keyw[eg][i];
          a = shamir_draw(k, te - K + 1, m.q, sh);
        } else {
          a = reduce_word(b.coeffs[(size_t)(d0 + eg) * t + (te - K)], m);
        }
      }
      coef[ew][ej][eg] = a;
    }
    __syncthreads();
    // ---- this wave's terms of the chunk: cnt from e0 on, the ns secret terms first ----
    const u32 e0 = ew0 + c * SH_JC;
    const u32 cnt = shamir_chunk_terms(ew0, Q, c, nt);
    const u32 ns = e0 < K ? (K - e0 < cnt ? K - e0 : cnt) : 0;
    if (PACKED) shamir_mac_loaded(acc, coef[wave], b.Lw + (size_t)e0 * cols + (live ? col : 0), cols, ns, live);
    for (u32 jj = ns; jj < cnt; ++jj) {
      u64 a[SH_DG];
#pragma unroll
      for (int g = 0; g < SH_DG; ++g) a[g] = coef[wave][jj][g];
#pragma unroll
      for (int g = 0; g < SH_DG; ++g) acc_mac_dev(acc[g], a[g], pw);
      pw = mulmod(pw, x, m);
    }
    __syncthreads();
  }
  // thread (g, lane) adds the four partial sums -- and, unpacked, the secret -- and stores dealer d0 + g's share of its party
  const u32 d = d0 + wave;
  const bool out = live && d < b.nd;
  const u64 s = shamir_meet(acc, part, !PACKED && out ? reduce_word(b.secrets[d], m) : 0, out, m);
  if (out) b.shares[(size_t)d * b.row_stride + party] = s;
}

// pack 0 is the unpacked entry points; pack >= 1 the packed ones, whatever pack
hipError_t launch_shamir_eval(const ShamirBatch& b, hipStream_t s) {
  if (b.nd == 0 || b.party_hi <= b.party_lo) return hipSuccess;
  const dim3 grid((b.party_hi - b.party_lo + 63) / 64, (b.nd + SH_DG - 1) / SH_DG);
  if (b.pack) shamir_eval_kernel<true><<<grid, dim3(256), 0, s>>>(b);
  else shamir_eval_kernel<false><<<grid, dim3(256), 0, s>>>(b);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ checked reconstruction
// The way back: out[s] = F_s(0) for the polynomial F_s of degree <= t through the basis columns 0..t of secret s, and every
// extra column t+1..count-1 compared with F_s at its point.  Both are one product shares[S][t+1] x W[t+1][T] over Z_p, with
// W[j][m] = L_j(x_m) the basis polynomial of column j at target m (target 0: x = 0; target m >= 1: the point of column t + m).
//
// Weights, barycentric: aux[j] = (prod_{i != j}(x_j - x_i))^-1 and aux[t + 1 + m] = prod_i (x_m - x_i), one wave per product
// (shamir_prod_kernel), then W[j][m] = aux[t + 1 + m] aux[j] (x_m - x_j)^-1 with one Fermat inversion per element
// (shamir_weights_kernel).  x_m - x_j is never 0: the points are distinct, below p, and 0 is no party's point.
// Interpolation: the frame of shamir_eval_kernel with the roles turned round.  A lane owns one target and SH_DG secrets; the
// four waves own the same 64 targets and secrets and a quarter of the t + 1 terms each.  The chunk's shares are wave-uniform:
// the workgroup stages them in LDS ([wave][term][secret], reduced below p) and lanes read them back as broadcasts, W[j][m] is
// one coalesced 8-byte load per lane and term, and the four partial sums meet in LDS.

// x[i] = index[i] + 1 for the indices of one launch's arguments: the indices are a HOST array of the caller's, and kernel
// arguments are the one way up that neither waits nor reads the array again when a captured call is replayed
__global__ __launch_bounds__(PVW_SHAMIR_POINTS) void shamir_points_kernel(ShamirPoints a) {
  if (threadIdx.x < a.n) a.x[threadIdx.x] = a.index[threadIdx.x] + 1;
}

// item e = blockIdx.x * 4 + wave of [0, count + 1): e <= t is basis column e (the product leaves i = e out and is inverted),
// e = t + 1 + m is target m.  64 lanes take the factors i = lane, lane + 64, ...; the 64 partial products meet in LDS.
__global__ __launch_bounds__(256) void shamir_prod_kernel(const u64* x, u64* aux, size_t count, u32 t, Mod m) {
  __shared__ u64 red[SH_WAVES][64];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t e = (size_t)blockIdx.x * SH_WAVES + wave;
  const bool live = e <= count;
  const bool basis = e <= t;
  u64 xe = 0;                                                    // target 0
  if (live && basis) xe = x[e];
  else if (live && e > (size_t)t + 1) xe = x[e - 1];             // target m >= 1 is column t + m = e - 1
  u64 prod = 1;
  if (live)
    for (u32 i = lane; i <= t; i += 64)
      if (!(basis && i == e)) prod = mulmod(prod, submod(xe, x[i], m.q), m);
  red[wave][lane] = prod;
  __syncthreads();
  if (lane == 0 && live) {
    u64 r = red[wave][0];
    for (u32 i = 1; i < 64; ++i) r = mulmod(r, red[wave][i], m);
    aux[e] = basis ? invmod_dev(r, m) : r;
  }
}

// one thread per element of W, the target fastest (W is row-major in the target)
__global__ __launch_bounds__(256) void shamir_weights_kernel(const u64* x, const u64* aux, u64* W, size_t count, u32 t, Mod m) {
  const size_t T = count - t;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= ((size_t)t + 1) * T) return;
  const size_t j = e / T, tm = e % T;
  const u64 xm = tm ? x[t + tm] : 0;
  const u64 inv = invmod_dev(submod(xm, x[j], m.q), m);
  W[e] = mulmod(mulmod(aux[(size_t)t + 1 + tm], aux[j], m), inv, m);
}

// Out[S][T] = A[S][terms] x W[terms][T] mod p for one workgroup (256 threads, block x = 64 targets, block y = SH_DG secrets):
// the frame both kernels below share.  A is any words at two strides, staged through LDS below p along whichever stride is the
// shorter one with neighbouring lanes; four weights are in flight ahead of their multiply-adds; the waves' partial sums meet in
// LDS.  Thread (wave, lane) comes back with the sum v of element (s = s0 + wave, tm) and whether that element exists.
// m by value: through a reference into the kernel's arguments the epilogue is compiled with 24 more 64-bit multiplies.
struct ShamirTile {
  u64 v;
  u32 s;
  size_t tm;
  bool live;
};
// MASKED: element (s, j) of A is staged as 0 where bit j of row s of `erased` is set -- the bit test stands beside
// the load.
template <bool MASKED = false>
__device__ __forceinline__ ShamirTile shamir_tile_product(const u64* A, size_t secret_stride, size_t term_stride, const u64* W, u32 ns,
                                                          u32 nt, u32 T, const Mod m, const u64* erased = nullptr, u32 ewords = 0) {
  __shared__ u64 sh[SH_WAVES][SH_JC][SH_DG];       // 8 KiB: the chunk of A, below p
  __shared__ u64 part[SH_WAVES][SH_DG][64];        // 8 KiB: the waves' partial sums, below p
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 s0 = blockIdx.y * SH_DG;
  const size_t tm = (size_t)blockIdx.x * 64 + lane;
  const bool live = tm < T;
  // wave w owns terms j = w * Q + [0, Q), cut off at nt; every wave walks the same number of chunks (barriers)
  const u32 Q = (nt + SH_WAVES - 1) / SH_WAVES;
  const u32 jw0 = wave * Q;
  const u32 nchunks = (Q + SH_JC - 1) / SH_JC;
  const bool term_fast = term_stride <= secret_stride;
  const u64* wcol = W + (live ? tm : 0);
  Acc acc[SH_DG];
#pragma unroll
  for (int g = 0; g < SH_DG; ++g) acc_zero(acc[g]);
  for (u32 c = 0; c < nchunks; ++c) {
    // ---- staging: entry e = (wave, term, secret) of the chunk, one per lane and trip ----
    for (u32 e = tid; e < SH_WAVES * SH_JC * SH_DG; e += 256) {
      const u32 ew = e / (SH_JC * SH_DG);
      const u32 ej = term_fast ? e % SH_JC : (e / SH_DG) % SH_JC;
      const u32 eg = term_fast ? (e / SH_JC) % SH_DG : e % SH_DG;
      const u32 off = c * SH_JC + ej;              // within the wave's range
      const u32 j = ew * Q + off;
      u64 a = 0;
      if (off < Q && j < nt && s0 + eg < ns) {
        if (!MASKED || !((erased[(size_t)(s0 + eg) * ewords + j / 64] >> (j % 64)) & 1))
          a = reduce_word(A[(size_t)(s0 + eg) * secret_stride + (size_t)j * term_stride], m);
      }
      sh[ew][ej][eg] = a;
    }
    __syncthreads();
    // ---- this wave's terms of the chunk ----
    const u32 j0 = jw0 + c * SH_JC;
    shamir_mac_loaded(acc, sh[wave], wcol + (size_t)j0 * T, T, shamir_chunk_terms(jw0, Q, c, nt), live);
    __syncthreads();
  }
  // thread (g, lane) adds the four partial sums of secret s0 + g at its target
  ShamirTile o;
  o.s = s0 + wave;                                 // SH_WAVES == SH_DG
  o.tm = tm;
  o.live = live && o.s < ns;
  o.v = shamir_meet(acc, part, 0, o.live, m);
  return o;
}

// The tile product of the shares' basis columns with W; target 0 is the secret, every other target is compared with the share
// of its column.  grid: x = blocks of 64 targets, y = groups of SH_DG secrets; 256 threads.
__global__ __launch_bounds__(256) void shamir_interp_kernel(ShamirInterp b) {
  const ShamirTile o = shamir_tile_product(b.shares, b.secret_stride, b.point_stride, b.W, b.ns, b.degree + 1, b.T, b.m);
  bool dev = false;
  if (o.live) {
    if (o.tm == 0) {
      b.out[o.s] = o.v;
    } else {
      const size_t col = (size_t)b.degree + o.tm;
      dev = reduce_word(b.shares[(size_t)o.s * b.secret_stride + col * b.point_stride], b.m) != o.v;
      if (dev && b.col_bad) atomicAdd(&b.col_bad[col], 1u);
    }
  }
  // one add per wave: the wave's lanes share the secret
  const u32 ndev = (u32)__popcll(__ballot(dev));
  if ((threadIdx.x & 63) == 0 && ndev && b.bad) atomicAdd(&b.bad[o.s], ndev);
}

// bad / col_bad start from 0 on every call and on every replay of a captured one: a kernel in stream order, not a memset node
// (DESIGN 8.7 found memset nodes not to clear on replay)
__global__ __launch_bounds__(256) void shamir_zero_counts_kernel(u32* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0;
}
hipError_t launch_shamir_zero_counts(u32* p, size_t n, hipStream_t s) {
  if (!p || !n) return hipSuccess;
  const size_t blocks = (n + 255) / 256;
  shamir_zero_counts_kernel<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s>>>(p, n);
  return hipGetLastError();
}

hipError_t launch_shamir_points(const u64* indices, size_t count, u64* x, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += PVW_SHAMIR_POINTS) {
    ShamirPoints a;
    a.n = (u32)(count - i0 < PVW_SHAMIR_POINTS ? count - i0 : PVW_SHAMIR_POINTS);
    for (u32 i = 0; i < PVW_SHAMIR_POINTS; ++i) a.index[i] = i < a.n ? indices[i0 + i] : 0;
    a.x = x + i0;
    shamir_points_kernel<<<dim3(1), dim3(PVW_SHAMIR_POINTS), 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ws: x [count] (filled by launch_shamir_points) | aux [count + 1] | W [t+1][count-t]
hipError_t launch_shamir_weights(u64* ws, size_t count, u32 t, const Mod& m, hipStream_t s) {
  const u64* x = ws;
  u64 *aux = ws + count, *W = aux + count + 1;
  shamir_prod_kernel<<<dim3((unsigned)((count + 1 + SH_WAVES - 1) / SH_WAVES)), dim3(256), 0, s>>>(x, aux, count, t, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t elems = ((size_t)t + 1) * (count - t);
  shamir_weights_kernel<<<dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s>>>(x, aux, W, count, t, m);
  return hipGetLastError();
}

// One launch per 65535 groups of secrets, which is what the grid's y dimension holds; from(s0) is b from secret s0 on.
template <class Args, class From>
static hipError_t launch_secret_groups(void (*kernel)(Args), const Args& b, From from, hipStream_t s) {
  if (b.ns == 0 || b.T == 0) return hipSuccess;
  const u32 per = 65535u * SH_DG;
  for (u32 s0 = 0; s0 < b.ns; s0 += per) {
    Args p = from(s0);
    p.ns = b.ns - s0 < per ? b.ns - s0 : per;
    kernel<<<dim3((b.T + 63) / 64, (p.ns + SH_DG - 1) / SH_DG), dim3(256), 0, s>>>(p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_shamir_interp(const ShamirInterp& b, hipStream_t s) {
  return launch_secret_groups(shamir_interp_kernel, b, [&](u32 s0) {
    ShamirInterp p = b;
    p.shares += (size_t)s0 * b.secret_stride;
    p.out += s0;
    if (p.bad) p.bad += s0;
    return p;
  }, s);
}

// ------------------------------------------------------------------------ corrected reconstruction
// The shares of one secret are a Reed-Solomon codeword of length count and dimension t + 1: with r = count - t - 1 redundant
// columns, up to E = r / 2 wrong shares per secret are found and left out, whichever columns hold them.  No column is a basis.
//   u_c = (prod_{i != c}(x_c - x_i))^-1 and lambda_c = u_c prod_{i != c}(-x_i)         (shamir_prod_kernel with t = count - 1)
//   V[c][j] = u_c x_c^j [count][r],  X[k][c] = x_c^k [E+1][count]                     (public, from the indices alone)
//   Synd = shares x V: all 0 for a row on one polynomial of degree <= t               (shamir_matmul_kernel)
//   inversion-free Berlekamp-Massey over a row's r syndromes -> the reversed locator Lambda_s, of degree L_s <= E, whose
//   roots are the points of the wrong columns                                          (shamir_bm_kernel)
//   M = Lambda x X: M[s][c] = Lambda_s(x_c)                                            (shamir_matmul_kernel)
//   the zeros of row s of M are the wrong columns; out[s] = (sum_c y_c lambda_c M[s][c]) / Lambda_s(0): Lagrange interpolation
//   at 0 of F_s Lambda_s (degree <= t + E <= count - 1) over ALL columns, where the wrong ones carry M = 0  (finish kernel)

// lambda_c = u_c P / (-x_c), P = prod_i(-x_i) = aux[count]; one thread per column
__global__ __launch_bounds__(256) void shamir_lambda_kernel(const u64* x, const u64* aux, u64* lam, u32 count, Mod m) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  lam[c] = mulmod(mulmod(aux[c], aux[count], m), invmod_dev(m.q - x[c], m), m);   // 0 < x_c < p
}

// one wave per column c: lane l starts at u_c x_c^l and steps by x_c^64, so a wave's stores to row c of V are coalesced
__global__ __launch_bounds__(256) void shamir_synd_weights_kernel(const u64* x, const u64* aux, u64* V, u32 count, u32 r, Mod m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 c = blockIdx.x * SH_WAVES + wave;
  if (c >= count) return;
  const u64 xc = x[c], step = powmod_dev(xc, 64u, m);
  u64 v = mulmod(aux[c], powmod_dev(xc, lane, m), m);
  u64* row = V + (size_t)c * r;
  for (u32 j = lane; j < r; j += 64) {
    row[j] = v;
    v = mulmod(v, step, m);
  }
}

// grid: x = blocks of 256 columns, y = blocks of 64 powers; a thread walks its 64 powers of x_c, lanes store along a row of X
__global__ __launch_bounds__(256) void shamir_powers_kernel(const u64* x, u64* X, u32 count, u32 nk, Mod m) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const u32 k0 = blockIdx.y * 64, k1 = k0 + 64 < nk ? k0 + 64 : nk;
  const u64 xc = x[c];
  u64 v = powmod_dev(xc, k0, m);
  for (u32 k = k0; k < k1; ++k) {
    X[(size_t)k * count + c] = v;
    v = mulmod(v, xc, m);
  }
}

// Out[S][T] = A[S][terms] x W[terms][T] mod p: the tile product, stored.
// grid: x = blocks of 64 targets, y = groups of SH_DG secrets; 256 threads.
__global__ __launch_bounds__(256) void shamir_matmul_kernel(ShamirMatmul b) {
  const ShamirTile o = shamir_tile_product(b.A, b.secret_stride, b.term_stride, b.W, b.ns, b.terms, b.T, b.m);
  if (o.live) b.out[(size_t)o.s * b.T + o.tm] = o.v;
}

// the sum of the lanes' values (each below p), the same in every lane
__device__ __forceinline__ u64 wave_addmod(u64 v, u64 q) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = addmod(v, (u64)__shfl_xor((unsigned long long)v, off), q);
  return v;
}

// One wave (one workgroup) per secret: inversion-free Berlekamp-Massey over the r syndromes of row s,
//   d = sum_{i <= L} C_i S_{n-i};  d != 0:  C <- b C - d x^m B  (and, when 2L <= n: B <- the old C, b <- d, L <- n + 1 - L).
// C and B lie in LDS, coefficient i with lane i % 64; the discrepancy is one lazy accumulator per lane, reduced, summed over
// the wave and so the same in every lane: every branch below is wave-uniform.  L never decreases, so the first update that
// would take it above E ends the row as undecodable, and E + 1 coefficients per polynomial are enough (deg x^m B <= the new L).
// The update walks the coefficients downwards in blocks of 64: B_{i-m} is read from this block or a lower one, which the
// walk has not overwritten yet.
// Out: lam[s][k] = C_{L-k} for k <= L, 0 up to E (all 0 for an undecodable row), and Lout[s] = L or PVW_SHAMIR_NO_LOCATOR.
__global__ __launch_bounds__(64) void shamir_bm_kernel(const u64* synd, u64* lam, u32* Lout, u32 r, u32 E, Mod m) {
  extern __shared__ u64 bm_lds[];                  // C [E + 1] | B [E + 1]
  u64 *C = bm_lds, *B = bm_lds + (E + 1);
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  const u64* S = synd + s * r;
  for (u32 i = lane; i <= E; i += 64) C[i] = B[i] = i == 0;
  __syncthreads();
  u32 L = 0, mm = 1;
  u64 bsc = 1;
  bool ok = true;
  for (u32 n = 0; n < r; ++n) {
    Acc a;
    acc_zero(a);
    for (u32 i = lane; i <= L; i += 64) acc_mac_dev(a, C[i], S[n - i]);      // L <= n
    const u64 d = wave_addmod(acc_reduce(a, m), m.q);
    if (d == 0) { ++mm; continue; }
    const bool grow = 2 * L <= n;
    const u32 Ln = grow ? n + 1 - L : L;
    if (Ln > E) { ok = false; break; }
    for (u32 k = Ln / 64 + 1; k-- > 0;) {
      const u32 i = k * 64 + lane;
      const bool in = i <= Ln;
      const u64 c = in ? C[i] : 0;
      const u64 bb = in && i >= mm ? B[i - mm] : 0;
      __syncthreads();
      if (in) {
        C[i] = submod(mulmod(bsc, c, m), mulmod(d, bb, m), m.q);
        if (grow) B[i] = c;
      }
      __syncthreads();
    }
    if (grow) { L = Ln; bsc = d; mm = 1; } else { ++mm; }
  }
  u64* row = lam + s * (E + 1);
  for (u32 k = lane; k <= E; k += 64) row[k] = ok && k <= L ? C[L - k] : 0;
  if (lane == 0) Lout[s] = ok ? L : PVW_SHAMIR_NO_LOCATOR;
}

// One wave (one workgroup) per secret over row s of M.  Pass 1 counts the zeros: a locator of degree L has at most L roots,
// and fewer than L among the points means no polynomial within E errors.  Pass 2: the ballot of the zeros of 64 columns is
// the mask word, every set bit one atomicAdd to its column's count (a consistent sharing issues none), and the other
// columns enter out[s] = (sum_c y_c lambda_c M[s][c]) Lambda_s(0)^-1.  Every mask word of the row is stored.
__global__ __launch_bounds__(64) void shamir_correct_finish_kernel(ShamirFinish f) {
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  const Mod m = f.m;
  const u32 count = f.count, words = (count + 63) / 64;
  const u32 L = f.L[s];
  const u64* Mrow = f.M + s * count;
  bool decodable = L != PVW_SHAMIR_NO_LOCATOR;
  if (decodable) {
    u32 nz = 0;
    for (u32 c0 = 0; c0 < count; c0 += 64) {
      const u32 c = c0 + lane;
      nz += (u32)__popcll(__ballot(c < count && Mrow[c] == 0));
    }
    decodable = nz == L;
  }
  if (!decodable) {
    if (f.mask)
      for (u32 w = lane; w < words; w += 64) f.mask[s * words + w] = 0;
    if (lane == 0) {
      f.out[s] = 0;
      if (f.nerr) f.nerr[s] = PVW_SHAMIR_NO_LOCATOR;
    }
    return;
  }
  Acc a;
  acc_zero(a);
  for (u32 c0 = 0; c0 < count; c0 += 64) {
    const u32 c = c0 + lane;
    const bool live = c < count;
    const u64 mv = live ? Mrow[c] : 1;
    const bool wrong = live && mv == 0;
    const u64 bal = __ballot(wrong);
    if (lane == 0 && f.mask) f.mask[s * words + c0 / 64] = bal;
    if (wrong && f.col_err) atomicAdd(&f.col_err[c], 1u);
    const u64 y = live && !wrong ? reduce_word(f.shares[s * f.secret_stride + (size_t)c * f.point_stride], m) : 0;
    acc_mac_dev(a, y, live ? mulmod(f.lam[c], mv, m) : 0);
  }
  const u64 v = wave_addmod(acc_reduce(a, m), m.q);
  if (lane == 0) {
    f.out[s] = mulmod(v, invmod_dev(f.Lam[s * (f.E + 1)], m), m);
    if (f.nerr) f.nerr[s] = L;
  }
}

// ws: x [count] (filled by launch_shamir_points) | aux [count + 1] | lambda [count] | V [count][r] | X [nk][count]
hipError_t launch_shamir_correct_weights(u64* ws, size_t count, u32 t, u32 nk, const Mod& m, hipStream_t s) {
  const u32 n = (u32)count, r = n - t - 1;
  const u64* x = ws;
  u64 *aux = ws + count, *lam = aux + count + 1, *V = lam + count, *X = V + count * r;
  shamir_prod_kernel<<<dim3((unsigned)((count + 1 + SH_WAVES - 1) / SH_WAVES)), dim3(256), 0, s>>>(x, aux, count, n - 1, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  shamir_lambda_kernel<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(x, aux, lam, n, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (r) {
    shamir_synd_weights_kernel<<<dim3((n + SH_WAVES - 1) / SH_WAVES), dim3(256), 0, s>>>(x, aux, V, n, r, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  shamir_powers_kernel<<<dim3((n + 255) / 256, (nk + 63) / 64), dim3(256), 0, s>>>(x, X, n, nk, m);
  return hipGetLastError();
}

hipError_t launch_shamir_matmul(const ShamirMatmul& b, hipStream_t s) {
  return launch_secret_groups(shamir_matmul_kernel, b, [&](u32 s0) {
    ShamirMatmul p = b;
    p.A += (size_t)s0 * b.secret_stride;
    p.out += (size_t)s0 * b.T;
    return p;
  }, s);
}

// E + 1 <= PVW_SHAMIR_MAX_LOCATOR: C and B of one wave fit the 64 KiB of LDS a launch gets without asking for more
hipError_t launch_shamir_bm(const u64* synd, u64* lam, u32* L, u32 ns, u32 r, const Mod& m, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  const u32 E = r / 2;
  shamir_bm_kernel<<<dim3(ns), dim3(64), (size_t)2 * (E + 1) * 8, s>>>(synd, lam, L, r, E, m);
  return hipGetLastError();
}

hipError_t launch_shamir_correct_finish(const ShamirFinish& f, u32 ns, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  shamir_correct_finish_kernel<<<dim3(ns), dim3(64), 0, s>>>(f);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ evaluation of the corrected polynomials
// values[s][j] = F_s(x*_j) behind the decode above, for any targets x*_j = targets[j] + 1.  G_s = F_s Lambda_s has degree
// <= t + E <= count - 1 and G_s(x_c) = y_c M[s][c] in every column (0 in the wrong ones), so G_s is interpolated through ALL
// columns, in barycentric form, and divided by the locator:
//   raw[s][j] = sum_i (y_i M[s][i]) C[i][j],  C[i][j] = u_i / (x*_j - x_i) (0 where x_i = x*_j)              (shamir_matmul_kernel)
//   scale_j = prod_{i : x_i != x*_j} (x*_j - x_i)
//   x*_j no column's point:        F_s(x*_j) = scale_j raw[s][j] / Lambda_s(x*_j)   (Lambda_s splits over the points: != 0)
//   x*_j = x_c, M[s][c] != 0:      F_s(x_c) = y_c
//   x*_j = x_c, M[s][c] == 0:      F_s(x_c) = G_s'(x_c) / Lambda_s'(x_c) = scale_j raw[s][j] / Lambda_s'(x_c): G_s / (x - x_c) through
//                                  the other count - 1 columns has the weights -u_i / u_c there, and scale_j = 1 / u_c
// Lambda_s and Lambda_s' at the targets are two more products, Lambda x Xt and Lambda x Xd with Xt[k][j] = x*_j^k and
// Xd[k][j] = k x*_j^(k-1).

// the product of the lanes' values (each below p), the same in every lane
__device__ __forceinline__ u64 wave_mulmod(u64 v, const Mod& m) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = mulmod(v, (u64)__shfl_xor((unsigned long long)v, off), m);
  return v;
}

// one wave per target j: scale_j, and the column whose point x*_j is (the points are distinct: at most one lane finds one, and
// PVW_SHAMIR_NO_COLUMN is the largest u32, so the minimum over the wave is that column or none).  Both meet by shuffles.
__global__ __launch_bounds__(256) void shamir_target_scale_kernel(const u64* x, const u64* xt, u64* scale, u32* coin, u32 count, u32 Tg,
                                                                  Mod m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 j = blockIdx.x * SH_WAVES + wave;
  if (j >= Tg) return;                                           // wave-uniform
  const u64 xs = xt[j];
  u64 prod = 1;
  u32 hit = PVW_SHAMIR_NO_COLUMN;
  for (u32 i = lane; i < count; i += 64) {
    const u64 d = submod(xs, x[i], m.q);
    if (d == 0) hit = i;
    else prod = mulmod(prod, d, m);
  }
  prod = wave_mulmod(prod, m);
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)hit, off);
    hit = o < hit ? o : hit;
  }
  if (lane == 0) {
    scale[j] = prod;
    coin[j] = hit;
  }
}

#define SH_CB 8      // columns per thread of the Cauchy matrix: one inversion for their SH_CB differences
// grid: x = blocks of 256 targets, y = blocks of SH_CB columns from i_base on; a thread owns one target and SH_CB columns, lanes
// store along a row of C.  The differences are inverted together (prefix products, one Fermat inversion, and back); a zero
// difference -- the target is that column's point -- enters the products as 1 and its entry is 0.
__global__ __launch_bounds__(256) void shamir_cauchy_kernel(const u64* x, const u64* aux, const u64* xt, u64* C, u32 i_base, u32 count,
                                                            u32 Tg, Mod m) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Tg) return;
  const u32 i0 = i_base + blockIdx.y * SH_CB;
  const u64 xs = xt[j];
  u64 d[SH_CB], pre[SH_CB];
  u64 run = 1;
#pragma unroll
  for (int b = 0; b < SH_CB; ++b) {
    const u32 i = i0 + b;
    d[b] = i < count ? submod(xs, x[i], m.q) : 0;
    pre[b] = run;
    run = mulmod(run, d[b] ? d[b] : 1, m);
  }
  u64 inv = invmod_dev(run, m);
#pragma unroll
  for (int b = SH_CB - 1; b >= 0; --b) {
    const u32 i = i0 + b;
    const u64 di = mulmod(inv, pre[b], m);           // d[b]^-1
    inv = mulmod(inv, d[b] ? d[b] : 1, m);
    if (i < count) C[(size_t)i * Tg + j] = d[b] ? mulmod(aux[i], di, m) : 0;
  }
}

// Xd[k][j] = k x_j^(k-1) (row 0 is 0), in the frame of shamir_powers_kernel
__global__ __launch_bounds__(256) void shamir_dpowers_kernel(const u64* x, u64* X, u32 count, u32 nk, Mod m) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const u32 k0 = blockIdx.y * 64, k1 = k0 + 64 < nk ? k0 + 64 : nk;
  const u64 xc = x[c];
  u64 v = k0 > 1 ? powmod_dev(xc, k0 - 1, m) : 1;    // x_c^(k-1) of the first k >= 1
  for (u32 k = k0; k < k1; ++k) {
    if (k == 0) { X[c] = 0; continue; }
    X[(size_t)k * count + c] = mulmod(reduce_word((u64)k, m), v, m);
    v = mulmod(v, xc, m);
  }
}

// YM[s][c] = y[s][c] M[s][c]: one thread per element, the column fastest
__global__ __launch_bounds__(256) void shamir_ym_kernel(const u64* shares, size_t secret_stride, size_t point_stride, const u64* M, u64* YM,
                                                        u32 ns, u32 count, Mod m) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)ns * count) return;
  const size_t s = e / count, c = e % count;
  const u64 mv = M[e];
  YM[e] = mv ? mulmod(reduce_word(shares[s * secret_stride + c * point_stride], m), mv, m) : 0;
}

// one thread per (s, j), the target fastest: picks the case, divides (one Fermat inversion) and stores
__global__ __launch_bounds__(256) void shamir_evaluate_finish_kernel(ShamirEvalFinish f) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)f.ns * f.Tg) return;
  const size_t s = e / f.Tg, j = e % f.Tg;
  const Mod m = f.m;
  u64 v = 0;
  if (f.nerr[s] != PVW_SHAMIR_NO_LOCATOR) {
    const u32 c = f.coin[j];
    if (c != PVW_SHAMIR_NO_COLUMN && f.M[s * f.count + c] != 0) {
      v = reduce_word(f.shares[s * f.secret_stride + (size_t)c * f.point_stride], m);
    } else {
      const u64 den = c != PVW_SHAMIR_NO_COLUMN ? f.LamD[e] : f.LamT[e];
      v = mulmod(mulmod(f.raw[e], f.scale[j], m), invmod_dev(den, m), m);
    }
  }
  f.values[s * f.value_stride + j] = v;
}

hipError_t launch_shamir_evaluate_weights(const u64* x, const u64* aux, u64* ws, size_t count, u32 nk, size_t Tg, const Mod& m,
                                          hipStream_t s) {
  const u32 n = (u32)count, tg = (u32)Tg;
  const u64* xt = ws;
  u64 *scale = ws + Tg, *C = scale + Tg, *Xt = C + count * Tg, *Xd = Xt + (size_t)nk * Tg;
  u32* coin = (u32*)(Xd + (size_t)nk * Tg);
  shamir_target_scale_kernel<<<dim3((tg + SH_WAVES - 1) / SH_WAVES), dim3(256), 0, s>>>(x, xt, scale, coin, n, tg, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const u32 per = 65535u * SH_CB;                  // the grid's y dimension
  for (u32 i0 = 0; i0 < n; i0 += per) {
    const u32 rows = n - i0 < per ? n - i0 : per;
    shamir_cauchy_kernel<<<dim3((tg + 255) / 256, (rows + SH_CB - 1) / SH_CB), dim3(256), 0, s>>>(x, aux, xt, C, i0, n, tg, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const dim3 grid((tg + 255) / 256, (nk + 63) / 64);
  shamir_powers_kernel<<<grid, dim3(256), 0, s>>>(xt, Xt, tg, nk, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  shamir_dpowers_kernel<<<grid, dim3(256), 0, s>>>(xt, Xd, tg, nk, m);
  return hipGetLastError();
}

hipError_t launch_shamir_ym(const u64* shares, size_t secret_stride, size_t point_stride, const u64* M, u64* YM, u32 ns, u32 count,
                            const Mod& m, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  const size_t blocks = ((size_t)ns * count + 255) / 256;
  shamir_ym_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(shares, secret_stride, point_stride, M, YM, ns, count, m);
  return hipGetLastError();
}

hipError_t launch_shamir_evaluate_finish(const ShamirEvalFinish& f, hipStream_t s) {
  if (f.ns == 0 || f.Tg == 0) return hipSuccess;
  const size_t blocks = ((size_t)f.ns * f.Tg + 255) / 256;
  shamir_evaluate_finish_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(f);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ reconstruction with erasures
// erased[s][W] flags the shares of row s that are known to be bad: eps_s of them, each costing ONE of the r redundant columns.
// The decode above with the erased shares read as 0 and a per-row erasure locator:
//   Synd = (shares o !erased) x V                                                       (shamir_matmul_masked_kernel)
//   Gamma_s(z) = prod_{c erased}(1 - x_c z);  T = Gamma_s Synd_s mod z^r, of which T_eps .. T_{r-1} are a sequence the error
//   locator Lambda_s alone generates; Berlekamp-Massey over those r - eps_s words with the bound E_s = (r - eps_s) / 2;
//   Psi_s = Gamma_s Lambda_s, reversed, of degree L_s = eps_s + deg Lambda_s <= r        (shamir_bm_erasures_kernel)
//   M = Psi x X with X [r+1][count]                                                      (shamir_matmul_kernel)
//   decodable iff row s of M has exactly L_s zeros (a root of Lambda_s on an erased point is a double root of Psi_s: fewer
//   distinct zeros); the zeros that are not erased are the wrong columns; out[s] as above with Psi_s(0)  (finish kernel)
// The evaluation of 8.13 runs unchanged with Psi_s in Lambda_s's place: an erased column carries M = 0 and is served by Psi_s'.
// The mask, Gamma, T and Psi follow from the mask and the indices alone or are as public as the locators of 8.11.

__global__ __launch_bounds__(256) void shamir_matmul_masked_kernel(ShamirMaskedMatmul b) {
  const ShamirTile o = shamir_tile_product<true>(b.A, b.secret_stride, b.term_stride, b.W, b.ns, b.terms, b.T, b.m, b.erased, b.ewords);
  if (o.live) b.out[(size_t)o.s * b.T + o.tm] = o.v;
}

// word w of a mask row of `count` columns, the padding bits of the last word cleared
__device__ __forceinline__ u64 shamir_erased_word(const u64* erow, u32 w, u32 count) {
  const u64 v = erow[w];
  return (w + 1) * 64 > count ? v & (((u64)1 << (count % 64)) - 1) : v;      // count % 64 != 0 there
}

// One wave (one workgroup) per secret.  LDS: Gamma [eps + 1] | C [E_s + 1] | B [E_s + 1], at most r + 3 words.
// Gamma grows by one factor per erased column, walked downwards in blocks of 64 like the update of shamir_bm_kernel.  T takes the
// place of Synd_s[eps ..] in global memory, blocks downwards: T_n reads Synd_s[n - eps .. n], which no earlier block has written.
// Then the recurrence of shamir_bm_kernel on T_eps .. T_{r-1}.  Every branch is wave-uniform (the mask words are read by all
// lanes alike, the discrepancy is the same in every lane).
// Out: psi[s][k] = Psi_{L_s - k} for k <= L_s, 0 up to r (all 0 for an undecodable row), Lout[s] = L_s or PVW_SHAMIR_NO_LOCATOR.
__global__ __launch_bounds__(64) void shamir_bm_erasures_kernel(u64* synd, const u64* erased, const u64* x, u64* psi, u32* Lout, u32 count,
                                                                u32 r, Mod m) {
  extern __shared__ u64 bme_lds[];
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  const u32 words = (count + 63) / 64;
  const u64* erow = erased + s * words;
  u64* S = synd + s * r;
  u64* row = psi + s * ((size_t)r + 1);
  u32 eps = 0;
  for (u32 w = 0; w < words; ++w) eps += (u32)__popcll(shamir_erased_word(erow, w, count));
  if (eps > r) {
    for (u32 k = lane; k <= r; k += 64) row[k] = 0;
    if (lane == 0) Lout[s] = PVW_SHAMIR_NO_LOCATOR;
    return;
  }
  u64* G = bme_lds;
  if (lane == 0) G[0] = 1;
  __syncthreads();
  u32 g = 0;                                                       // deg Gamma so far
  for (u32 w = 0; w < words; ++w) {
    u64 word = shamir_erased_word(erow, w, count);
    while (word) {
      const u64 xc = x[w * 64 + (u32)__builtin_ctzll(word)];
      word &= word - 1;
      for (u32 k = (g + 1) / 64 + 1; k-- > 0;) {                   // Gamma_i <- Gamma_i - x_c Gamma_{i-1}, i <= g + 1
        const u32 i = k * 64 + lane;
        const bool in = i <= g + 1;
        const u64 cur = in && i <= g ? G[i] : 0;
        const u64 prev = in && i >= 1 ? G[i - 1] : 0;
        __syncthreads();
        if (in) G[i] = submod(cur, mulmod(xc, prev, m), m.q);
        __syncthreads();
      }
      ++g;
    }
  }
  const u32 nT = r - eps, E = nT / 2;
  if (eps)
    for (u32 k = (nT + 63) / 64; k-- > 0;) {
      const u32 idx = k * 64 + lane, n = eps + idx;
      const bool live = idx < nT;
      Acc a;
      acc_zero(a);
      for (u32 i = 0; i <= eps; ++i) acc_mac_dev(a, G[i], live ? S[n - i] : 0);
      const u64 v = acc_reduce(a, m);
      __syncthreads();
      if (live) S[n] = v;
      __syncthreads();
    }
  const u64* T = S + eps;
  u64 *C = G + eps + 1, *B = C + E + 1;
  for (u32 i = lane; i <= E; i += 64) C[i] = B[i] = i == 0;
  __syncthreads();
  u32 L = 0, mm = 1;
  u64 bsc = 1;
  bool ok = true;
  for (u32 n = 0; n < nT; ++n) {
    Acc a;
    acc_zero(a);
    for (u32 i = lane; i <= L; i += 64) acc_mac_dev(a, C[i], T[n - i]);      // L <= n
    const u64 d = wave_addmod(acc_reduce(a, m), m.q);
    if (d == 0) { ++mm; continue; }
    const bool grow = 2 * L <= n;
    const u32 Ln = grow ? n + 1 - L : L;
    if (Ln > E) { ok = false; break; }
    for (u32 k = Ln / 64 + 1; k-- > 0;) {
      const u32 i = k * 64 + lane;
      const bool in = i <= Ln;
      const u64 c = in ? C[i] : 0;
      const u64 bb = in && i >= mm ? B[i - mm] : 0;
      __syncthreads();
      if (in) {
        C[i] = submod(mulmod(bsc, c, m), mulmod(d, bb, m), m.q);
        if (grow) B[i] = c;
      }
      __syncthreads();
    }
    if (grow) { L = Ln; bsc = d; mm = 1; } else { ++mm; }
  }
  // Psi_j = sum_i Lambda_i Gamma_{j-i}, stored at k = L_s - j
  const u32 Ls = eps + L;
  for (u32 k = lane; k <= r; k += 64) {
    u64 v = 0;
    if (ok && k <= Ls) {
      const u32 j = Ls - k;
      Acc a;
      acc_zero(a);
      for (u32 i = j > eps ? j - eps : 0; i <= L && i <= j; ++i) acc_mac_dev(a, C[i], G[j - i]);
      v = acc_reduce(a, m);
    }
    row[k] = v;
  }
  if (lane == 0) Lout[s] = ok ? Ls : PVW_SHAMIR_NO_LOCATOR;
}

// shamir_correct_finish_kernel for a row with erasures: the zeros of M's row must number exactly L_s, the erased ones among them;
// the mask word is the ballot of the zeros without the erased word, nerr = L_s - eps_s, and out[s] divides by Psi_s(0) = f.Lam[s][0]
// (rows f.E + 1 = r + 1 words apart).  No share at an erased position enters: M is 0 there.
__global__ __launch_bounds__(64) void shamir_erasures_finish_kernel(ShamirFinish f, const u64* erased) {
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  const Mod m = f.m;
  const u32 count = f.count, words = (count + 63) / 64;
  const u32 L = f.L[s];
  const u64* Mrow = f.M + s * count;
  const u64* erow = erased + s * words;
  bool decodable = L != PVW_SHAMIR_NO_LOCATOR;
  u32 eps = 0;
  if (decodable) {
    u32 nz = 0;
    for (u32 c0 = 0; c0 < count; c0 += 64) {
      const u32 c = c0 + lane;
      nz += (u32)__popcll(__ballot(c < count && Mrow[c] == 0));
      eps += (u32)__popcll(shamir_erased_word(erow, c0 / 64, count));
    }
    decodable = nz == L;
  }
  if (!decodable) {
    if (f.mask)
      for (u32 w = lane; w < words; w += 64) f.mask[s * words + w] = 0;
    if (lane == 0) {
      f.out[s] = 0;
      if (f.nerr) f.nerr[s] = PVW_SHAMIR_NO_LOCATOR;
    }
    return;
  }
  Acc a;
  acc_zero(a);
  for (u32 c0 = 0; c0 < count; c0 += 64) {
    const u32 c = c0 + lane;
    const bool live = c < count;
    const u64 mv = live ? Mrow[c] : 1;
    const bool zero = live && mv == 0;
    const u64 bal = __ballot(zero) & ~shamir_erased_word(erow, c0 / 64, count);
    const bool wrong = (bal >> lane) & 1;
    if (lane == 0 && f.mask) f.mask[s * words + c0 / 64] = bal;
    if (wrong && f.col_err) atomicAdd(&f.col_err[c], 1u);
    const u64 y = live && !zero ? reduce_word(f.shares[s * f.secret_stride + (size_t)c * f.point_stride], m) : 0;
    acc_mac_dev(a, y, live ? mulmod(f.lam[c], mv, m) : 0);
  }
  const u64 v = wave_addmod(acc_reduce(a, m), m.q);
  if (lane == 0) {
    f.out[s] = mulmod(v, invmod_dev(f.Lam[s * ((size_t)f.E + 1)], m), m);
    if (f.nerr) f.nerr[s] = L - eps;
  }
}

// One wave per 64 words of one row: trip k packs the 64 columns of word w0 + k by ballot and lane k keeps it, so the wave's
// store runs along the row.  The loads follow the caller's strides.  block = row * wb + block of words.
__global__ __launch_bounds__(64) void shamir_erasure_mask_kernel(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound,
                                                                 u32 count, u32 wb, size_t secret_stride, size_t point_stride, u64* mask) {
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x / wb;
  const u32 words = (count + 63) / 64, w0 = (blockIdx.x % wb) * 64;
  const u32 nw = words - w0 < 64 ? words - w0 : 64;
  u64 mine = 0;
  for (u32 k = 0; k < nw; ++k) {
    const u32 c = (w0 + k) * 64 + lane;
    bool e = false;
    if (c < count) {
      const size_t off = s * secret_stride + (size_t)c * point_stride;
      if (status) e = (status[off] & status_bits) != 0;
      if (noise) e = e || noise[off] > noise_bound;
    }
    const u64 bal = __ballot(e);
    if (lane == k) mine = bal;
  }
  if (lane < nw) mask[s * words + w0 + lane] = mine;
}

hipError_t launch_shamir_matmul_masked(const ShamirMaskedMatmul& b, hipStream_t s) {
  return launch_secret_groups(shamir_matmul_masked_kernel, b, [&](u32 s0) {
    ShamirMaskedMatmul p = b;
    p.A += (size_t)s0 * b.secret_stride;
    p.out += (size_t)s0 * b.T;
    p.erased += (size_t)s0 * b.ewords;
    return p;
  }, s);
}

// r + 1 <= PVW_SHAMIR_MAX_LOCATOR: Gamma, C and B of one wave take at most r + 3 words of LDS
hipError_t launch_shamir_bm_erasures(u64* synd, const u64* erased, const u64* x, u64* psi, u32* L, u32 ns, u32 count, u32 r, const Mod& m,
                                     hipStream_t s) {
  if (ns == 0) return hipSuccess;
  shamir_bm_erasures_kernel<<<dim3(ns), dim3(64), ((size_t)r + 3) * 8, s>>>(synd, erased, x, psi, L, count, r, m);
  return hipGetLastError();
}

hipError_t launch_shamir_erasures_finish(const ShamirFinish& f, const u64* erased, u32 ns, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  shamir_erasures_finish_kernel<<<dim3(ns), dim3(64), 0, s>>>(f, erased);
  return hipGetLastError();
}

hipError_t launch_shamir_erasure_mask(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound, u32 count, u32 ns,
                                      size_t secret_stride, size_t point_stride, u64* mask, hipStream_t s) {
  if (ns == 0 || count == 0) return hipSuccess;
  const u32 words = (count + 63) / 64, wb = (words + 63) / 64;
  const u32 per = 0x7FFFFFFFu / wb;                                // rows per launch: what the grid's x dimension holds
  for (u32 s0 = 0; s0 < ns; s0 += per) {
    const u32 rows = ns - s0 < per ? ns - s0 : per;
    shamir_erasure_mask_kernel<<<dim3(rows * wb), dim3(64), 0, s>>>(status ? status + (size_t)s0 * secret_stride : nullptr,
                                                                    noise ? noise + (size_t)s0 * secret_stride : nullptr, status_bits,
                                                                    noise_bound, count, wb, secret_stride, point_stride,
                                                                    mask + (size_t)s0 * words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ------------------------------------------------------------------------ the weights of packed shares
// L_j(x) = w_j prod_{m != j}(x + m) with w_j = ((-1)^j j! (K-1-j)!)^-1: the denominators are factorials, so ONE inversion, of
// (K-1)!, and a walk down give every 1/j!, and no element of Lw needs one.  x + m <= n + K - 1 < p is never 0.

// one workgroup: thread 0 walks the factorials (2K multiplies and the inversion), then w[j] = (-1)^j / (j! (K-1-j)!)
__global__ __launch_bounds__(256) void shamir_packed_basis_kernel(u64* w, u64* invf, u32 K, Mod m) {
  if (threadIdx.x == 0) {
    u64 f = 1;
    for (u32 j = 2; j < K; ++j) f = mulmod(f, (u64)j, m);        // (K-1)!, K - 1 < p
    u64 inv = invmod_dev(f, m);
    for (u32 j = K - 1;; --j) {
      invf[j] = inv;                                               // 1 / j!
      if (j == 0) break;
      inv = mulmod(inv, (u64)j, m);
    }
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < K; j += 256) {
    const u64 v = mulmod(invf[j], invf[K - 1 - j], m);             // never 0
    w[j] = (j & 1) ? m.q - v : v;
  }
}

// one thread per column i (x = party_lo + i + 1), lanes store along the rows of Lw: a suffix pass leaves prod_{m>j}(x + m) in
// Lw[j][i] (and Z(x) / x = prod_{m>=1}(x + m) in zt[i]), a prefix pass multiplies prod_{m<j}(x + m) and w_j in
__global__ __launch_bounds__(256) void shamir_packed_weights_kernel(u64* Lw, u64* zt, const u64* w, u32 K, u32 party_lo, u32 cols,
                                                                    Mod m) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cols) return;
  const u64 x = (u64)party_lo + i + 1;
  u64 suf = 1;
  for (u32 j = K; j-- > 0;) {
    Lw[(size_t)j * cols + i] = suf;
    suf = mulmod(suf, x + j, m);
  }
  zt[i] = Lw[i];                                                   // row 0: prod_{m=1..K-1}(x + m)
  u64 pre = 1;
  for (u32 j = 0; j < K; ++j) {
    u64* e = Lw + (size_t)j * cols + i;
    *e = mulmod(mulmod(*e, pre, m), w[j], m);
    pre = mulmod(pre, x + j, m);
  }
}

// ws: Lw [K][cols] | zt [cols] | w [K] | 1/j! [K] (shamir_packed_words)
hipError_t launch_shamir_packed_weights(u64* ws, u32 pack, u32 party_lo, u32 party_hi, const Mod& m, hipStream_t s) {
  if (pack == 0 || party_hi <= party_lo) return hipSuccess;
  const u32 cols = party_hi - party_lo;
  u64 *Lw = ws, *zt = Lw + (size_t)pack * cols, *w = zt + cols, *invf = w + pack;
  shamir_packed_basis_kernel<<<dim3(1), dim3(256), 0, s>>>(w, invf, pack, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  shamir_packed_weights_kernel<<<dim3((cols + 255) / 256), dim3(256), 0, s>>>(Lw, zt, w, pack, party_lo, cols, m);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ shares over a prime below 2^256
// shares[d][i] = f_d(i + 1) mod p with elements of four words (pvw_wide.h).  The point x = i + 1 is below 2^32, so the
// polynomial is walked by Horner from the top coefficient, acc <- acc x + a_e for e = t .. 0 (a_0 the secret): one wide_step
// per term, 8 + 8 v_mad_u64_u32 and one correction, where a power-and-product walk would pay a general 256 x 256-bit product.
// A lane owns one party of one dealer; the 256 lanes of a workgroup own 256 parties and walk ALL t + 1 terms -- no term split:
// partial sums of a split would have to be multiplied by a power of x at the meet, which is the general product again.
// Coefficients are uniform across the workgroup: each chunk of SHW_JC terms is made in LDS, one lane per coefficient (drawn
// from the dealer's key, or an input word reduced), scaled and below pn, and read back as broadcasts; every workgroup of a
// dealer repeats the draw for its 256 parties (one ChaCha8 block or so per lane against 256 steps per lane).  Nothing but
// the result reaches memory: the share's four words, or its limbs as rows of the pass's scratch.
#define SHW_JC 256   // terms per staging chunk: one per lane

// grid: x = blocks of 256 parties of [party_lo, party_hi), y = the launch's dealers; 256 threads.
__global__ __launch_bounds__(256) void shamir_eval_wide_kernel(ShamirWideBatch b) {
  __shared__ u64 coef[SHW_JC][4];                  // 8 KiB: the chunk's coefficients, scaled, below pn
  __shared__ u32 keyw[8];
  const u32 tid = threadIdx.x;
  const WideMod m = b.m;
  const u32 t = b.degree, nt = t + 1;
  const u32 dx = blockIdx.y, d = b.d_lo + dx;
  const u32 col = blockIdx.x * 256 + tid;
  const u32 party = b.party_lo + col;
  const bool live = col < b.party_hi - b.party_lo;
  const bool drawn = b.coeffs == nullptr && t != 0;
  if (drawn && tid == 0) {
    ChaChaKey k;
    if (b.rnd) k = call_seed(b.rnd->seed, b.rnd->counter + b.rnd_off + (u64)dx * b.key_stride);   // derived when the kernel runs
    else k = b.key[dx];
#pragma unroll
    for (int i = 0; i < 8; ++i) keyw[i] = k.w[i];
  }
  __syncthreads();
  const u32 x = live ? party + 1 : 1;              // x <= n < 2^32
  u64 acc[4] = {0, 0, 0, 0};
  const u32 nchunks = (nt + SHW_JC - 1) / SHW_JC;
  for (u32 c = 0; c < nchunks; ++c) {
    // ---- staging: slot tid holds term e = t - c * SHW_JC - tid, the terms in the order Horner takes them ----
    const u32 first = c * SHW_JC;                  // terms taken before this chunk
    u64 a[4] = {0, 0, 0, 0};
    if (first + tid < nt) {
      const u32 e = t - first - tid;
      if (e == 0) {
        wide_reduce_scaled(b.secrets + (size_t)d * 4, m, a);
      } else if (drawn) {
        ChaChaKey k;
#pragma unroll
        for (int i = 0; i < 8; ++i) k.w[i] = keyw[i];
        wide_draw_scaled(k, DOM_SHAMIR, e, m, a);
      } else {
        wide_reduce_scaled(b.coeffs + ((size_t)d * t + (e - 1)) * 4, m, a);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) coef[tid][i] = a[i];
    __syncthreads();
    const u32 cnt = nt - first < SHW_JC ? nt - first : SHW_JC;
    for (u32 jj = 0; jj < cnt; ++jj) {
      u64 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = coef[jj][i];
      wide_step(acc, x, v, m);
    }
    __syncthreads();
  }
  if (!live) return;
  wide_shr(acc, m.shift);                          // the share, below p
  if (b.num_limbs == 0) {
    u64* o = b.out + ((size_t)d * b.row_stride + party) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = acc[i];
    return;
  }
  const u64 mask = ((u64)1 << b.limb_bits) - 1;
  for (u32 w = 0; w < b.num_limbs; ++w) {
    const u64 v = (u64)d * b.num_limbs + w;
    if (v >= b.v0 && v < (u64)b.v0 + b.nv) b.out[(size_t)(v - b.v0) * b.row_stride + party] = acc[0] & mask;
    wide_shr(acc, b.limb_bits);                    // limb_bits < 64
  }
}

hipError_t launch_shamir_eval_wide(const ShamirWideBatch& b, hipStream_t s) {
  if (b.nd == 0 || b.party_hi <= b.party_lo) return hipSuccess;
  shamir_eval_wide_kernel<<<dim3((b.party_hi - b.party_lo + 255) / 256, b.nd), dim3(256), 0, s>>>(b);
  return hipGetLastError();
}

// the step alone on operands of the caller's, scaled on the way in and back on the way out
__global__ __launch_bounds__(256) void shamir_wide_step_kernel(WideMod m, const u64* acc, const u64* x, const u64* add, size_t count,
                                                               u64* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  u64 a[4], v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { a[k] = acc[i * 4 + k]; v[k] = add[i * 4 + k]; }
  wide_shl(a, m.shift);
  wide_shl(v, m.shift);
  wide_step(a, (u32)x[i], v, m);
  wide_shr(a, m.shift);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = a[k];
}
hipError_t launch_shamir_wide_step(const WideMod& m, const u64* acc, const u64* x, const u64* add, size_t count, u64* out, hipStream_t s) {
  if (!count) return hipSuccess;
  shamir_wide_step_kernel<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s>>>(m, acc, x, add, count, out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ checked reconstruction below 2^256
// The contract and the layout of 8.10 with elements of four words: columns 0..t are the basis, T = count - t targets (target 0
// is x = 0, target m >= 1 the point of column t + m), out[s] = F_s(0) and every extra share is compared with F_s at its point.
// Arithmetic: Montgomery's product of pvw_wide.h.  The workspace (points, products, weights) is public and holds everything
// times R = 2^256; the shares stay plain, and share * (W R) reduced once is the plain share * W.
// Weights: aux as in 8.10, one wave per product (shamir_prod_wide_kernel; a basis column's product is inverted by Fermat, about
// 380 products on one lane), then W[j][m] = aux[t+1+m] aux[j] (x_m - x_j)^-1.  An inversion per element would cost 380 products
// against the half product per secret that the element is used for below, so SHW_WG = 32 entries of one target (rows j0 .. j0+31)
// share one inversion by Montgomery's trick: the running products of the differences go out to the entries' own slots of W,
// the last one is inverted, and the walk back turns every slot into its weight -- 3 products an entry for the trick, 2 for
// the weight, 380 / 32 = 12 for its part of the inversion.  No register holds a prefix: the group size costs no VGPRs.
// Product: the frame of shamir_tile_product.  A lane owns one target and SHW_SG secrets; the four waves own the same 64 targets
// and secrets and a quarter of the t + 1 terms each.  The chunk's shares are staged in LDS below p ([wave][term][secret]) and
// read back as broadcasts; W[j][m] is two coalesced 16-byte loads per lane and term, the next term's in flight.  A term is a
// 16-digit schoolbook product (64 v_mad_u64_u32) ADDED to an unreduced accumulator that wide_acc_add keeps below p 2^256 with
// one conditional subtraction; the accumulator is reduced ONCE, when the wave's terms are done.  Partial sums are field
// elements, so the waves' four meet in LDS by plain additions mod p.
#define SHW_SG 4      // secrets per lane
#define SHW_TC 8      // terms per wave and staging chunk
#define SHW_WG 32     // entries of W that share one inversion
static_assert(SHW_SG == SH_WAVES && SHW_SG == SH_DG, "the last phase maps one wave to one secret of the group; launch_secret_groups");

// the workspace's elements are 32-byte aligned: two 16-byte accesses
__device__ __forceinline__ void wide_ld(const u64* p, u64 (&v)[4]) {
  const ulonglong2 lo = ((const ulonglong2*)p)[0], hi = ((const ulonglong2*)p)[1];
  v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
}
__device__ __forceinline__ void wide_st(u64* p, const u64 (&v)[4]) {
  ((ulonglong2*)p)[0] = make_ulonglong2(v[0], v[1]);
  ((ulonglong2*)p)[1] = make_ulonglong2(v[2], v[3]);
}

// x[i] = (index[i] + 1) R mod p (the indices travel as kernel arguments, shamir_points_kernel)
__global__ __launch_bounds__(PVW_SHAMIR_POINTS) void shamir_points_wide_kernel(ShamirPoints a, WideMont m) {
  if (threadIdx.x >= a.n) return;
  const u64 i = a.index[threadIdx.x];
  const u64 x[4] = {i + 1, i + 1 == 0 ? (u64)1 : (u64)0, 0, 0};
  u64 xm[4];
  wide_mont_in(x, m, xm);
  wide_st(a.x + (size_t)threadIdx.x * 4, xm);
}

// shamir_prod_kernel over four words: item e = blockIdx.x * 4 + wave of [0, count + 1)
__global__ __launch_bounds__(256) void shamir_prod_wide_kernel(const u64* x, u64* aux, size_t count, u32 t, WideMont m) {
  __shared__ u64 red[SH_WAVES][64][4];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t e = (size_t)blockIdx.x * SH_WAVES + wave;
  const bool live = e <= count;
  const bool basis = e <= t;
  u64 xe[4] = {0, 0, 0, 0};                                      // target 0
  if (live && basis) wide_ld(x + e * 4, xe);
  else if (live && e > (size_t)t + 1) wide_ld(x + (e - 1) * 4, xe);
  u64 prod[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) prod[k] = m.one[k];
  if (live)
    for (u32 i = lane; i <= t; i += 64)
      if (!(basis && i == e)) {
        u64 xi[4], d[4];
        wide_ld(x + (size_t)i * 4, xi);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = xe[k];
        wide_sub_p(d, xi, m);
        wide_mont_mul(prod, d, m, prod);
      }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[wave][lane][k] = prod[k];
  __syncthreads();
  if (lane == 0 && live) {
    for (u32 i = 1; i < 64; ++i) {
      u64 f[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = red[wave][i][k];
      wide_mont_mul(prod, f, m, prod);
    }
    if (basis) wide_mont_inv(prod, m, prod);
    wide_st(aux + e * 4, prod);
  }
}

// one thread per target and group of SHW_WG rows, the target fastest: thread e = group * T + target
__global__ __launch_bounds__(256) void shamir_weights_wide_kernel(const u64* x, const u64* aux, u64* W, size_t count, u32 t, WideMont m) {
  const size_t T = count - t;
  const size_t groups = ((size_t)t + SHW_WG) / SHW_WG;           // ceil((t + 1) / SHW_WG)
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= groups * T) return;
  const size_t tm = e % T, j0 = (e / T) * SHW_WG;
  const u32 cnt = (size_t)t + 1 - j0 < SHW_WG ? (u32)((size_t)t + 1 - j0) : SHW_WG;
  u64 xm[4] = {0, 0, 0, 0};
  if (tm) wide_ld(x + ((size_t)t + tm) * 4, xm);
  // forward: slot k <- d_0 ... d_k, d_k = x_m - x_{j0+k} (never 0: distinct points below p, and 0 is no party's point)
  u64 run[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) run[k] = m.one[k];
  for (u32 k = 0; k < cnt; ++k) {
    u64 xj[4], d[4];
    wide_ld(x + (j0 + k) * 4, xj);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = xm[i];
    wide_sub_p(d, xj, m);
    wide_mont_mul(run, d, m, run);
    wide_st(W + ((j0 + k) * T + tm) * 4, run);
  }
  u64 inv[4], lm[4];
  wide_mont_inv(run, m, inv);                                    // (d_0 ... d_{cnt-1})^-1
  wide_ld(aux + ((size_t)t + 1 + tm) * 4, lm);
  // back: inv = (d_0 ... d_k)^-1 on entry to step k; d_k^-1 = inv * slot[k-1]
  for (u32 k = cnt; k-- > 0;) {
    u64 xj[4], d[4], pre[4], wj[4], dinv[4];
    wide_ld(x + (j0 + k) * 4, xj);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = xm[i];
    wide_sub_p(d, xj, m);
    if (k) wide_ld(W + ((j0 + k - 1) * T + tm) * 4, pre);
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[i] = m.one[i];
    }
    wide_mont_mul(inv, pre, m, dinv);
    wide_mont_mul(inv, d, m, inv);
    wide_ld(aux + (j0 + k) * 4, wj);
    wide_mont_mul(wj, lm, m, wj);
    wide_mont_mul(wj, dinv, m, wj);
    wide_st(W + ((j0 + k) * T + tm) * 4, wj);
  }
}

// Out[S][T][4] = A[S][terms][4] x W[terms][T][4] mod p for one workgroup (256 threads, block x = 64 targets, block y = SHW_SG
// secrets): the frame shamir_interp_wide_kernel and shamir_matmul_wide_kernel share, as shamir_tile_product serves the one-word
// family.  A is any words at two strides (in elements), staged below p; W is stored times R.  Thread (wave, lane) comes back with
// the plain sum v of element (s = s0 + wave, tm) and whether that element exists.
struct ShamirWideTile {
  u64 v[4];
  u32 s;
  size_t tm;
  bool live;
};
// MASKED: element (s, j) of A is staged as 0 where bit j of row s of `erased` is set -- the bit test stands beside
// the load, so an erased element is not loaded.
template <bool MASKED = false>
__device__ __forceinline__ ShamirWideTile shamir_tile_product_wide(const u64* A, size_t secret_stride, size_t term_stride, const u64* W,
                                                                   u32 ns, u32 nt, u32 T, const WideMont m, const u64* erased = nullptr,
                                                                   u32 ewords = 0) {
  __shared__ u64 sh[SH_WAVES][SHW_TC][SHW_SG][4];  // 4 KiB: the chunk of A, below p
  __shared__ u64 part[SH_WAVES][SHW_SG][64][4];    // 32 KiB: the waves' partial sums, below p
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 s0 = blockIdx.y * SHW_SG;
  const size_t tm = (size_t)blockIdx.x * 64 + lane;
  const bool live = tm < T;
  // wave w owns terms j = w * Q + [0, Q), cut off at nt; every wave walks the same number of chunks (barriers)
  const u32 Q = (nt + SH_WAVES - 1) / SH_WAVES;
  const u32 jw0 = wave * Q;
  const u32 nchunks = (Q + SHW_TC - 1) / SHW_TC;
  const bool term_fast = term_stride <= secret_stride;
  const u64* wcol = W + (live ? tm : 0) * 4;
  u32 acc[SHW_SG][16];                             // each below p 2^256 (wide_acc_add)
#pragma unroll
  for (int g = 0; g < SHW_SG; ++g) wide_acc_zero(acc[g]);
  for (u32 c = 0; c < nchunks; ++c) {
    // ---- staging: entry e = (wave, term, secret) of the chunk, one per lane of the first two waves ----
    if (tid < SH_WAVES * SHW_TC * SHW_SG) {
      const u32 e = tid;
      const u32 ew = e / (SHW_TC * SHW_SG);
      const u32 ej = term_fast ? e % SHW_TC : (e / SHW_SG) % SHW_TC;
      const u32 eg = term_fast ? (e / SHW_TC) % SHW_SG : e % SHW_SG;
      const u32 off = c * SHW_TC + ej;             // within the wave's range
      const u32 j = ew * Q + off;
      u64 a[4] = {0, 0, 0, 0};
      if (off < Q && j < nt && s0 + eg < ns && (!MASKED || !((erased[(size_t)(s0 + eg) * ewords + j / 64] >> (j % 64)) & 1))) {
        const u64* sp = A + ((size_t)(s0 + eg) * secret_stride + (size_t)j * term_stride) * 4;
        const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
        wide_reduce_p(w, m, a);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) sh[ew][ej][eg][k] = a[k];
    }
    __syncthreads();
    // ---- this wave's terms of the chunk ----
    const u32 lo = c * SHW_TC;
    u32 cnt = lo < Q ? (Q - lo < SHW_TC ? Q - lo : SHW_TC) : 0;
    const u32 j0 = jw0 + lo;
    if (j0 >= nt) cnt = 0;
    else if (nt - j0 < cnt) cnt = nt - j0;
    u64 w[4] = {0, 0, 0, 0};
    if (cnt) wide_ld(wcol + (size_t)j0 * T * 4, w);
    for (u32 jj = 0; jj < cnt; ++jj) {
      u64 wn[4] = {0, 0, 0, 0};
      if (jj + 1 < cnt) wide_ld(wcol + (size_t)(j0 + jj + 1) * T * 4, wn);
#pragma unroll
      for (int g = 0; g < SHW_SG; ++g) {
        u64 a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = sh[wave][jj][g][k];
        u32 P[16];
        wide_mul_full(a, w, P);
        wide_acc_add(acc[g], P, m);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = wn[k];
    }
    __syncthreads();
  }
  // every wave reduces its sums once; thread (g, lane) adds the four partial sums of secret s0 + g at its target
#pragma unroll
  for (int g = 0; g < SHW_SG; ++g) {
    u64 r[4];
    wide_redc(acc[g], m, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) part[wave][g][lane][k] = r[k];
  }
  __syncthreads();
  ShamirWideTile o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o.v[k] = part[0][wave][lane][k];
#pragma unroll
  for (int ww = 1; ww < SH_WAVES; ++ww) {
    u64 f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = part[ww][wave][lane][k];
    wide_add_p(o.v, f, m);
  }
  o.s = s0 + wave;                                 // SH_WAVES == SHW_SG
  o.tm = tm;
  o.live = live && o.s < ns;
  return o;
}

// The tile product of the shares' basis columns with W; target 0 is the secret, every other target is compared with the share
// of its column.  grid: x = blocks of 64 targets, y = groups of SHW_SG secrets; 256 threads.
__global__ __launch_bounds__(256) void shamir_interp_wide_kernel(ShamirInterpWide b) {
  const WideMont m = b.m;
  const ShamirWideTile o = shamir_tile_product_wide(b.shares, b.secret_stride, b.point_stride, b.W, b.ns, b.degree + 1, b.T, m);
  const u32 s = o.s;
  bool dev = false;
  if (o.live) {
    if (o.tm == 0) {
      u64* out = b.out + (size_t)s * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = o.v[k];
    } else {
      const size_t col = (size_t)b.degree + o.tm;
      const u64* sp = b.shares + ((size_t)s * b.secret_stride + col * b.point_stride) * 4;
      const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
      u64 y[4];
      wide_reduce_p(w, m, y);
      dev = (y[0] != o.v[0]) | (y[1] != o.v[1]) | (y[2] != o.v[2]) | (y[3] != o.v[3]);
      if (dev && b.col_bad) atomicAdd(&b.col_bad[col], 1u);
    }
  }
  // one add per wave: the wave's lanes share the secret
  const u32 ndev = (u32)__popcll(__ballot(dev));
  if ((threadIdx.x & 63) == 0 && ndev && b.bad) atomicAdd(&b.bad[s], ndev);
}

hipError_t launch_shamir_points_wide(const u64* indices, size_t count, u64* x, const WideMont& m, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += PVW_SHAMIR_POINTS) {
    ShamirPoints a;
    a.n = (u32)(count - i0 < PVW_SHAMIR_POINTS ? count - i0 : PVW_SHAMIR_POINTS);
    for (u32 i = 0; i < PVW_SHAMIR_POINTS; ++i) a.index[i] = i < a.n ? indices[i0 + i] : 0;
    a.x = x + i0 * 4;
    shamir_points_wide_kernel<<<dim3(1), dim3(PVW_SHAMIR_POINTS), 0, s>>>(a, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ws: x [count][4] (filled by launch_shamir_points_wide) | aux [count + 1][4] | W [t+1][count-t][4]
hipError_t launch_shamir_weights_wide(u64* ws, size_t count, u32 t, const WideMont& m, hipStream_t s) {
  const u64* x = ws;
  u64 *aux = ws + count * 4, *W = aux + (count + 1) * 4;
  shamir_prod_wide_kernel<<<dim3((unsigned)((count + 1 + SH_WAVES - 1) / SH_WAVES)), dim3(256), 0, s>>>(x, aux, count, t, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t threads = (((size_t)t + SHW_WG) / SHW_WG) * (count - t);
  shamir_weights_wide_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(x, aux, W, count, t, m);
  return hipGetLastError();
}

hipError_t launch_shamir_interp_wide(const ShamirInterpWide& b, hipStream_t s) {
  return launch_secret_groups(shamir_interp_wide_kernel, b, [&](u32 s0) {
    ShamirInterpWide p = b;
    p.shares += (size_t)s0 * b.secret_stride * 4;
    p.out += (size_t)s0 * 4;
    if (p.bad) p.bad += s0;
    return p;
  }, s);
}

// One lane per element, by the host routine's own walk (pvw_shamir_wide_from_limbs_host): Horner over the limbs from the top,
// acc <- acc 2^limb_bits + limb in two steps with multipliers below 2^32, every limb word read mod p first.
__global__ __launch_bounds__(256) void shamir_wide_fold_kernel(WideMod m, const u64* limbs, size_t count, size_t limb_stride,
                                                               size_t elem_stride, u32 limb_bits, u32 num_limbs, u64* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const u32 h0 = limb_bits / 2, h1 = limb_bits - h0;
  u64 acc[4] = {0, 0, 0, 0};
  const u64 zero[4] = {0, 0, 0, 0};
  for (u32 w = num_limbs; w-- > 0;) {
    u64 add[4];
    wide_reduce_word_scaled(limbs[(size_t)w * limb_stride + i * elem_stride], m, add);
    wide_step(acc, 1u << h0, zero, m);
    wide_step(acc, 1u << h1, add, m);
  }
  wide_shr(acc, m.shift);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = acc[k];
}
hipError_t launch_shamir_wide_fold(const WideMod& m, const u64* limbs, size_t count, size_t limb_stride, size_t elem_stride, u32 limb_bits,
                                   u32 num_limbs, u64* out, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += (size_t)1 << 30) {      // what one grid's x dimension carries with room to spare
    const size_t cnt = count - i0 < ((size_t)1 << 30) ? count - i0 : (size_t)1 << 30;
    shamir_wide_fold_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s>>>(m, limbs + i0 * elem_stride, cnt, limb_stride,
                                                                                    elem_stride, limb_bits, num_limbs, out + i0 * 4);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// the product alone on operands of the caller's
__global__ __launch_bounds__(256) void shamir_wide_mul_kernel(WideMont m, const u64* a, const u64* b, size_t count, u64* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  u64 x[4], y[4], r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { x[k] = a[i * 4 + k]; y[k] = b[i * 4 + k]; }
  wide_mul(x, y, m, r);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = r[k];
}
hipError_t launch_shamir_wide_mul(const WideMont& m, const u64* a, const u64* b, size_t count, u64* out, hipStream_t s) {
  if (!count) return hipSuccess;
  shamir_wide_mul_kernel<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s>>>(m, a, b, count, out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ corrected reconstruction below 2^256
// The decode of 8.11 step by step, with elements of four words and the product of pvw_wide.h.  Forms (R = 2^256):
//   x, aux (u_c, then prod_i(-x_i)), lambda, V, X        public, stored times R
//   shares, Synd = shares x V                            plain: REDC(plain * (V R)) is the plain product
//   C, B, b, Lambda                                      times R: the locator is the operand that meets plain syndromes
//   M = Lambda x X                                       times R: REDC((Lambda R)(X R)); its zero test does not depend on the form
//   out                                                  plain: (sum_c y_c REDC((lambda_c R)(M_c R))) reduced once, then times
//                                                        (Lambda_s(0) R)^-1 R by one more REDC
#define SHW_LG 16     // columns of lambda that share one inversion

// a^e times R for a times R; the exponent's bits from the top
__device__ __forceinline__ void wide_mont_pow(const u64 (&a)[4], u32 e, const WideMont& m, u64 (&out)[4]) {
  u64 r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = m.one[k];
  for (int b = 31 - __builtin_clz(e | 1); b >= 0; --b) {
    wide_mont_mul(r, r, m, r);
    if ((e >> b) & 1) wide_mont_mul(r, a, m, r);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = r[k];
}

// lambda_c = u_c P / (-x_c), P = prod_i(-x_i) = aux[count].  One thread per group of SHW_LG columns, which share one Fermat
// inversion by Montgomery's trick (shamir_weights_wide_kernel): the running products of -x_c go out to the columns' own slots of
// lam, the last one is inverted, and the walk back turns every slot into its weight.
__global__ __launch_bounds__(64) void shamir_lambda_wide_kernel(const u64* x, const u64* aux, u64* lam, u32 count, WideMont m) {
  const u32 g = blockIdx.x * 64 + threadIdx.x;
  const u32 c0 = g * SHW_LG;
  if (c0 >= count) return;
  const u32 cnt = count - c0 < SHW_LG ? count - c0 : SHW_LG;
  const u64 zero[4] = {0, 0, 0, 0};
  u64 run[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) run[k] = m.one[k];
  for (u32 k = 0; k < cnt; ++k) {
    u64 xc[4], d[4] = {0, 0, 0, 0};
    wide_ld(x + (size_t)(c0 + k) * 4, xc);
    wide_sub_p(d, xc, m);                                        // -x_c, never 0: 0 < x_c < p
    wide_mont_mul(run, d, m, run);
    wide_st(lam + (size_t)(c0 + k) * 4, run);
  }
  u64 inv[4], P[4];
  wide_mont_inv(run, m, inv);
  wide_ld(aux + (size_t)count * 4, P);
  for (u32 k = cnt; k-- > 0;) {
    u64 xc[4], d[4], pre[4], u[4], dinv[4];
    wide_ld(x + (size_t)(c0 + k) * 4, xc);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = zero[i];
    wide_sub_p(d, xc, m);
    if (k) wide_ld(lam + (size_t)(c0 + k - 1) * 4, pre);
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[i] = m.one[i];
    }
    wide_mont_mul(inv, pre, m, dinv);                            // (-x_c)^-1
    wide_mont_mul(inv, d, m, inv);
    wide_ld(aux + (size_t)(c0 + k) * 4, u);
    wide_mont_mul(u, P, m, u);
    wide_mont_mul(u, dinv, m, u);
    wide_st(lam + (size_t)(c0 + k) * 4, u);
  }
}

// one wave per column c: lane l starts at u_c x_c^l and steps by x_c^64, so a wave's stores to row c of V are coalesced
__global__ __launch_bounds__(256) void shamir_synd_weights_wide_kernel(const u64* x, const u64* aux, u64* V, u32 count, u32 r, WideMont m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 c = blockIdx.x * SH_WAVES + wave;
  if (c >= count) return;
  u64 xc[4], step[4], v[4], u[4];
  wide_ld(x + (size_t)c * 4, xc);
  wide_ld(aux + (size_t)c * 4, u);
  wide_mont_pow(xc, 64u, m, step);
  wide_mont_pow(xc, lane, m, v);
  wide_mont_mul(v, u, m, v);
  u64* row = V + (size_t)c * r * 4;
  for (u32 j = lane; j < r; j += 64) {
    wide_st(row + (size_t)j * 4, v);
    wide_mont_mul(v, step, m, v);
  }
}

// grid: x = blocks of 256 columns, y = blocks of 64 powers; a thread walks its 64 powers of x_c, lanes store along a row of X
__global__ __launch_bounds__(256) void shamir_powers_wide_kernel(const u64* x, u64* X, u32 count, u32 nk, WideMont m) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const u32 k0 = blockIdx.y * 64, k1 = k0 + 64 < nk ? k0 + 64 : nk;
  u64 xc[4], v[4];
  wide_ld(x + (size_t)c * 4, xc);
  wide_mont_pow(xc, k0, m, v);
  for (u32 k = k0; k < k1; ++k) {
    wide_st(X + ((size_t)k * count + c) * 4, v);
    wide_mont_mul(v, xc, m, v);
  }
}

// Out[S][T][4] = A[S][terms][4] x W[terms][T][4] mod p: the wide tile product, stored.
// grid: x = blocks of 64 targets, y = groups of SHW_SG secrets; 256 threads.
__global__ __launch_bounds__(256) void shamir_matmul_wide_kernel(ShamirMatmulWide b) {
  const ShamirWideTile o = shamir_tile_product_wide(b.A, b.secret_stride, b.term_stride, b.W, b.ns, b.terms, b.T, b.m);
  if (o.live) wide_st(b.out + ((size_t)o.s * b.T + o.tm) * 4, o.v);
}

// the sum of the lanes' values (each below p), the same in every lane
__device__ __forceinline__ void wave_add_wide(u64 (&v)[4], const WideMont& m) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    u64 f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = (u64)__shfl_xor((unsigned long long)v[k], off);
    wide_add_p(v, f, m);
  }
}
__device__ __forceinline__ bool wide_zero(const u64 (&v)[4]) { return !(v[0] | v[1] | v[2] | v[3]); }

// shamir_bm_kernel over four words: one wave (one workgroup) per secret, inversion-free Berlekamp-Massey over the r syndromes of
// row s,  d = sum_{i <= L} C_i S_{n-i};  d != 0:  C <- b C - d x^m B  (and, when 2L <= n: B <- the old C, b <- d, L <- n + 1 - L).
// C and B lie in dynamic LDS, each as four planes of E + 1 words (word k of coefficient i at plane k, slot i), so that the lanes
// of one access are consecutive words; coefficient i belongs to lane i % 64.  C, B and b are kept times R, the syndromes are
// plain: a term C_i S_{n-i} is wide_mul_full of (C_i R) < p and S_{n-i} < p, so every product is below p p < p R and
// wide_acc_add's invariant (one operand below p, the other below R) holds term by term: the lane's accumulator stays below
// p 2^256 however many terms it takes, and ONE wide_redc gives the lane's plain part of d.  The parts are summed over the wave by
// shuffles and wide_add_p, so d is the same in every lane and every branch is wave-uniform.  d R = REDC(d r2) once per step;
// the update's two products are REDC((b R)(C_i R)) and REDC((d R)(B_j R)), each with both operands below p.
// L never decreases: the first update that would take it above E ends the row as undecodable.  The update walks downwards in
// blocks of 64: B_{i-m} is read from this block or a lower one, which the walk has not overwritten yet.
// Out: lam[s][k] = C_{L-k} R for k <= L, 0 up to E (all 0 for an undecodable row), and Lout[s] = L or PVW_SHAMIR_NO_LOCATOR.
__global__ __launch_bounds__(64) void shamir_bm_wide_kernel(const u64* synd, u64* lam, u32* Lout, u32 r, u32 E, WideMont m) {
  extern __shared__ u64 bmw_lds[];                 // C [4][E + 1] | B [4][E + 1]
  const u32 nE = E + 1;
  u64 *C = bmw_lds, *B = bmw_lds + (size_t)4 * nE;
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  const u64* S = synd + s * r * 4;
  for (u32 i = lane; i <= E; i += 64)
#pragma unroll
    for (int k = 0; k < 4; ++k) C[k * nE + i] = B[k * nE + i] = i == 0 ? m.one[k] : 0;
  __syncthreads();
  u32 L = 0, mm = 1;
  u64 bsc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) bsc[k] = m.one[k];
  bool ok = true;
  for (u32 n = 0; n < r; ++n) {
    u32 acc[16];
    wide_acc_zero(acc);
    for (u32 i = lane; i <= L; i += 64) {          // L <= n
      u64 c[4], sv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = C[k * nE + i];
      wide_ld(S + (size_t)(n - i) * 4, sv);
      u32 P[16];
      wide_mul_full(c, sv, P);
      wide_acc_add(acc, P, m);
    }
    u64 d[4];
    wide_redc(acc, m, d);
    wave_add_wide(d, m);
    if (wide_zero(d)) { ++mm; continue; }
    const bool grow = 2 * L <= n;
    const u32 Ln = grow ? n + 1 - L : L;
    if (Ln > E) { ok = false; break; }
    wide_mont_in(d, m, d);
    for (u32 k = Ln / 64 + 1; k-- > 0;) {
      const u32 i = k * 64 + lane;
      const bool in = i <= Ln;
      u64 c[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
      if (in) {
#pragma unroll
        for (int w = 0; w < 4; ++w) c[w] = C[w * nE + i];
        if (i >= mm) {
#pragma unroll
          for (int w = 0; w < 4; ++w) bb[w] = B[w * nE + i - mm];
        }
      }
      __syncthreads();
      if (in) {
        u64 v[4], t[4];
        wide_mont_mul(bsc, c, m, v);
        wide_mont_mul(d, bb, m, t);
        wide_sub_p(v, t, m);
#pragma unroll
        for (int w = 0; w < 4; ++w) C[w * nE + i] = v[w];
        if (grow) {
#pragma unroll
          for (int w = 0; w < 4; ++w) B[w * nE + i] = c[w];
        }
      }
      __syncthreads();
    }
    if (grow) {
      L = Ln;
      mm = 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) bsc[k] = d[k];
    } else {
      ++mm;
    }
  }
  u64* row = lam + s * nE * 4;
  for (u32 k = lane; k <= E; k += 64) {
    u64 v[4] = {0, 0, 0, 0};
    if (ok && k <= L) {
#pragma unroll
      for (int w = 0; w < 4; ++w) v[w] = C[w * nE + L - k];
    }
    wide_st(row + (size_t)k * 4, v);
  }
  if (lane == 0) Lout[s] = ok ? L : PVW_SHAMIR_NO_LOCATOR;
}

// v, held in two vector registers from here on (the compiler would keep a wave-uniform value in scalar ones)
__device__ __forceinline__ u64 wide_in_vgpr(u64 v) {
  u32 lo = (u32)v, hi = (u32)(v >> 32);
  asm volatile("" : "+v"(lo), "+v"(hi));
  return ((u64)hi << 32) | lo;
}

// shamir_correct_finish_kernel over four words: one wave (one workgroup) per secret over row s of M.  Pass 1 counts the zeros
// (four zero words: the same test whether the element is stored times R or not); fewer than L means no polynomial within E
// errors.  Pass 2: the ballot of the zeros of 64 columns is the mask word, every set bit one atomicAdd to its column's count, and
// the other columns enter out[s] = (sum_c y_c lambda_c M[s][c]) Lambda_s(0)^-1: the weight REDC((lambda_c R)(M R)) is below p and
// the share is reduced below p, so the lane's accumulator stays below p 2^256 (wide_acc_add) and is reduced once.
__global__ __launch_bounds__(64) void shamir_correct_finish_wide_kernel(ShamirFinishWide f) {
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  // r2 and one travel in vector registers: held in scalar ones beside the kernel's thirteen arguments and the carries of the
  // products they cost 32 spilled SGPRs
  WideMont m = f.m;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m.r2[k] = wide_in_vgpr(m.r2[k]);
    m.one[k] = wide_in_vgpr(m.one[k]);
  }
  const u32 count = f.count, words = (count + 63) / 64;
  const u32 L = f.L[s];
  const u64* Mrow = f.M + s * count * 4;
  bool decodable = L != PVW_SHAMIR_NO_LOCATOR;
  if (decodable) {
    u32 nz = 0;
    for (u32 c0 = 0; c0 < count; c0 += 64) {
      const u32 c = c0 + lane;
      u64 mv[4] = {1, 0, 0, 0};
      if (c < count) wide_ld(Mrow + (size_t)c * 4, mv);
      nz += (u32)__popcll(__ballot(wide_zero(mv)));
    }
    decodable = nz == L;
  }
  if (!decodable) {
    if (f.mask)
      for (u32 w = lane; w < words; w += 64) f.mask[s * words + w] = 0;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) f.out[s * 4 + k] = 0;          // the caller's buffer: word stores, as the checked kernel's
      if (f.nerr) f.nerr[s] = PVW_SHAMIR_NO_LOCATOR;
    }
    return;
  }
  u32 acc[16];
  wide_acc_zero(acc);
  for (u32 c0 = 0; c0 < count; c0 += 64) {
    const u32 c = c0 + lane;
    const bool live = c < count;
    u64 mv[4] = {1, 0, 0, 0};
    if (live) wide_ld(Mrow + (size_t)c * 4, mv);
    const bool wrong = wide_zero(mv);
    const u64 bal = __ballot(wrong);
    if (lane == 0 && f.mask) f.mask[s * words + c0 / 64] = bal;
    if (wrong && f.col_err) atomicAdd(&f.col_err[c], 1u);
    if (live && !wrong) {
      const u64* sp = f.shares + (s * f.secret_stride + (size_t)c * f.point_stride) * 4;
      const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
      u64 y[4], lw[4];
      wide_reduce_p(w, m, y);
      wide_ld(f.lam + (size_t)c * 4, lw);
      wide_mont_mul(lw, mv, m, lw);
      u32 P[16];
      wide_mul_full(y, lw, P);
      wide_acc_add(acc, P, m);
    }
  }
  u64 v[4];
  wide_redc(acc, m, v);
  wave_add_wide(v, m);
  if (lane == 0) {
    u64 l0[4];
    wide_ld(f.Lam + s * (f.E + 1) * 4, l0);
    wide_mont_inv(l0, m, l0);
    wide_mont_mul(v, l0, m, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) f.out[s * 4 + k] = v[k];
    if (f.nerr) f.nerr[s] = L;
  }
}

// ws: x [count][4] (filled by launch_shamir_points_wide) | aux [count + 1][4] | lambda [count][4] | V [count][r][4] | X [nk][count][4]
hipError_t launch_shamir_correct_weights_wide(u64* ws, size_t count, u32 t, u32 nk, const WideMont& m, hipStream_t s) {
  const u32 n = (u32)count, r = n - t - 1;
  const u64* x = ws;
  u64 *aux = ws + count * 4, *lam = aux + (count + 1) * 4, *V = lam + count * 4, *X = V + count * r * 4;
  shamir_prod_wide_kernel<<<dim3((unsigned)((count + 1 + SH_WAVES - 1) / SH_WAVES)), dim3(256), 0, s>>>(x, aux, count, n - 1, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const u32 groups = (n + SHW_LG - 1) / SHW_LG;
  shamir_lambda_wide_kernel<<<dim3((groups + 63) / 64), dim3(64), 0, s>>>(x, aux, lam, n, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (r) {
    shamir_synd_weights_wide_kernel<<<dim3((n + SH_WAVES - 1) / SH_WAVES), dim3(256), 0, s>>>(x, aux, V, n, r, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  shamir_powers_wide_kernel<<<dim3((n + 255) / 256, (nk + 63) / 64), dim3(256), 0, s>>>(x, X, n, nk, m);
  return hipGetLastError();
}

hipError_t launch_shamir_matmul_wide(const ShamirMatmulWide& b, hipStream_t s) {
  return launch_secret_groups(shamir_matmul_wide_kernel, b, [&](u32 s0) {
    ShamirMatmulWide p = b;
    p.A += (size_t)s0 * b.secret_stride * 4;
    p.out += (size_t)s0 * b.T * 4;
    return p;
  }, s);
}

// ------------------------------------------------------------------------ erasures below 2^256
// The decode of 8.16 with elements of four words, in the forms of 8.20: x, V, X, Gamma, the locators, Psi and M are times R; the
// shares, the syndromes and the Forney syndromes are plain.
//   Synd = (shares o !erased) x V                                                       (shamir_matmul_masked_wide_kernel)
//   Gamma_s, T = Gamma_s Synd_s mod z^r in place, Berlekamp-Massey over T_eps .. T_{r-1} with the bound E_s = (r - eps_s) / 2,
//   Psi_s = Gamma_s Lambda_s reversed, L_s = eps_s + deg Lambda_s                       (shamir_bm_erasures_wide_kernel)
//   M = Psi x X with X [r+1][count]                                                      (shamir_matmul_wide_kernel)
//   decodable iff row s of M has exactly L_s zeros; the zeros that are not erased are the wrong columns   (finish kernel)
// The mask, Gamma, T and Psi are as public as the locators of 8.20.

__global__ __launch_bounds__(256) void shamir_matmul_masked_wide_kernel(ShamirMaskedMatmulWide b) {
  const ShamirWideTile o =
      shamir_tile_product_wide<true>(b.A, b.secret_stride, b.term_stride, b.W, b.ns, b.terms, b.T, b.m, b.erased, b.ewords);
  if (o.live) wide_st(b.out + ((size_t)o.s * b.T + o.tm) * 4, o.v);
}

// shamir_bm_erasures_kernel over four words: one wave (one workgroup) per secret.
// Dynamic LDS: Gamma [eps + 1] | C [E_s + 1] | B [E_s + 1], at most r + 3 elements, each polynomial as four planes of words (word
// k of coefficient i at plane k, slot i) so that the lanes of one access touch consecutive words, as in shamir_bm_wide_kernel.
// Gamma grows by one factor (1 - x_c z) per set bit of the row's mask words, walked downwards in blocks of 64; it is kept times
// R: Gamma_i R <- Gamma_i R - REDC((x_c R)(Gamma_{i-1} R)) with x_c R from the points buffer, both operands below p.
// T takes the place of Synd_s[eps ..] in global memory, blocks downwards: T_n = sum_{i <= eps} Gamma_i S_{n-i} reads
// Synd_s[n - eps .. n], which no earlier (higher) block has written, and the block's own stores wait behind a barrier for its
// loads.  A term is wide_mul_full of (Gamma_i R) < p and the plain S_{n-i} < p (a tile product's output, wide_add_p's result),
// so every product is below p p < p R and wide_acc_add's invariant (accumulator and addend below p R) holds term by term
// however large eps is; ONE wide_redc then gives the plain T_n < p.
// Then the recurrence of shamir_bm_wide_kernel on T_eps .. T_{r-1} with the bound E_s, its invariants word for word: C, B and b
// times R, T plain.  Psi_j = sum_i Lambda_i Gamma_{j-i}, a lane per coefficient: a term is wide_mul_full of (Lambda_i R) < p and
// (Gamma_{j-i} R) < p, below p p again, and one wide_redc leaves Psi_j R.
// Every branch that holds a barrier is wave-uniform: the mask words are read by all lanes alike and the discrepancy is the same
// in every lane; only the tail of a block (a lane past the last coefficient) is predicated, between the barriers.
// Out: psi[s][k] = Psi_{L_s - k} R for k <= L_s, 0 up to r (all 0 for an undecodable row: eps_s > r or deg Lambda_s > E_s),
// Lout[s] = L_s or PVW_SHAMIR_NO_LOCATOR.
__global__ __launch_bounds__(64) void shamir_bm_erasures_wide_kernel(u64* synd, const u64* erased, const u64* x, u64* psi, u32* Lout,
                                                                     u32 count, u32 r, WideMont m) {
  extern __shared__ u64 bmew_lds[];
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  const u32 words = (count + 63) / 64;
  const u64* erow = erased + s * words;
  u64* S = synd + s * r * 4;
  u64* row = psi + s * ((size_t)r + 1) * 4;
  u32 eps = 0;
  for (u32 w = 0; w < words; ++w) eps += (u32)__popcll(shamir_erased_word(erow, w, count));
  if (eps > r) {
    const u64 z[4] = {0, 0, 0, 0};
    for (u32 k = lane; k <= r; k += 64) wide_st(row + (size_t)k * 4, z);
    if (lane == 0) Lout[s] = PVW_SHAMIR_NO_LOCATOR;
    return;
  }
  const u32 nG = eps + 1;
  u64* G = bmew_lds;
  for (u32 i = lane; i <= eps; i += 64)
#pragma unroll
    for (int k = 0; k < 4; ++k) G[k * nG + i] = i == 0 ? m.one[k] : 0;
  __syncthreads();
  u32 g = 0;                                                       // deg Gamma so far
  for (u32 w = 0; w < words; ++w) {
    u64 word = shamir_erased_word(erow, w, count);
    while (word) {
      u64 xc[4];
      wide_ld(x + (size_t)(w * 64 + (u32)__builtin_ctzll(word)) * 4, xc);
      word &= word - 1;
      for (u32 k = (g + 1) / 64 + 1; k-- > 0;) {                   // Gamma_i <- Gamma_i - x_c Gamma_{i-1}, i <= g + 1
        const u32 i = k * 64 + lane;
        const bool in = i <= g + 1;
        u64 cur[4] = {0, 0, 0, 0}, prev[4] = {0, 0, 0, 0};
        if (in && i <= g) {
#pragma unroll
          for (int q = 0; q < 4; ++q) cur[q] = G[q * nG + i];
        }
        if (in && i >= 1) {
#pragma unroll
          for (int q = 0; q < 4; ++q) prev[q] = G[q * nG + i - 1];
        }
        __syncthreads();
        if (in) {
          u64 t[4];
          wide_mont_mul(xc, prev, m, t);
          wide_sub_p(cur, t, m);
#pragma unroll
          for (int q = 0; q < 4; ++q) G[q * nG + i] = cur[q];
        }
        __syncthreads();
      }
      ++g;
    }
  }
  const u32 nT = r - eps, E = nT / 2, nE = E + 1;
  if (eps)
    for (u32 k = (nT + 63) / 64; k-- > 0;) {
      const u32 idx = k * 64 + lane, n = eps + idx;
      const bool live = idx < nT;
      u32 acc[16];
      wide_acc_zero(acc);
      if (live)
        for (u32 i = 0; i <= eps; ++i) {
          u64 gi[4], sv[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) gi[q] = G[q * nG + i];
          wide_ld(S + (size_t)(n - i) * 4, sv);
          u32 P[16];
          wide_mul_full(gi, sv, P);
          wide_acc_add(acc, P, m);
        }
      u64 v[4];
      wide_redc(acc, m, v);
      __syncthreads();
      if (live) wide_st(S + (size_t)n * 4, v);
      __syncthreads();
    }
  const u64* T = S + (size_t)eps * 4;
  u64 *C = G + (size_t)4 * nG, *B = C + (size_t)4 * nE;
  for (u32 i = lane; i <= E; i += 64)
#pragma unroll
    for (int k = 0; k < 4; ++k) C[k * nE + i] = B[k * nE + i] = i == 0 ? m.one[k] : 0;
  __syncthreads();
  u32 L = 0, mm = 1;
  u64 bsc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) bsc[k] = m.one[k];
  bool ok = true;
  for (u32 n = 0; n < nT; ++n) {
    u32 acc[16];
    wide_acc_zero(acc);
    for (u32 i = lane; i <= L; i += 64) {          // L <= n
      u64 c[4], sv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = C[k * nE + i];
      wide_ld(T + (size_t)(n - i) * 4, sv);
      u32 P[16];
      wide_mul_full(c, sv, P);
      wide_acc_add(acc, P, m);
    }
    u64 d[4];
    wide_redc(acc, m, d);
    wave_add_wide(d, m);
    if (wide_zero(d)) { ++mm; continue; }
    const bool grow = 2 * L <= n;
    const u32 Ln = grow ? n + 1 - L : L;
    if (Ln > E) { ok = false; break; }
    wide_mont_in(d, m, d);
    for (u32 k = Ln / 64 + 1; k-- > 0;) {
      const u32 i = k * 64 + lane;
      const bool in = i <= Ln;
      u64 c[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
      if (in) {
#pragma unroll
        for (int w = 0; w < 4; ++w) c[w] = C[w * nE + i];
        if (i >= mm) {
#pragma unroll
          for (int w = 0; w < 4; ++w) bb[w] = B[w * nE + i - mm];
        }
      }
      __syncthreads();
      if (in) {
        u64 v[4], t[4];
        wide_mont_mul(bsc, c, m, v);
        wide_mont_mul(d, bb, m, t);
        wide_sub_p(v, t, m);
#pragma unroll
        for (int w = 0; w < 4; ++w) C[w * nE + i] = v[w];
        if (grow) {
#pragma unroll
          for (int w = 0; w < 4; ++w) B[w * nE + i] = c[w];
        }
      }
      __syncthreads();
    }
    if (grow) {
      L = Ln;
      mm = 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) bsc[k] = d[k];
    } else {
      ++mm;
    }
  }
  // Psi_j = sum_i Lambda_i Gamma_{j-i}, stored at k = L_s - j
  const u32 Ls = eps + L;
  for (u32 k = lane; k <= r; k += 64) {
    u64 v[4] = {0, 0, 0, 0};
    if (ok && k <= Ls) {
      const u32 j = Ls - k;
      u32 acc[16];
      wide_acc_zero(acc);
      for (u32 i = j > eps ? j - eps : 0; i <= L && i <= j; ++i) {
        u64 ci[4], gj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ci[q] = C[q * nE + i];
          gj[q] = G[q * nG + j - i];
        }
        u32 P[16];
        wide_mul_full(ci, gj, P);
        wide_acc_add(acc, P, m);
      }
      wide_redc(acc, m, v);
    }
    wide_st(row + (size_t)k * 4, v);
  }
  if (lane == 0) Lout[s] = ok ? Ls : PVW_SHAMIR_NO_LOCATOR;
}

// shamir_correct_finish_wide_kernel for a row with erasures: the zeros of M's row must number exactly L_s, the erased ones among
// them; the mask word is the ballot of the zeros without the erased word, nerr = L_s - eps_s, and out[s] divides by
// Psi_s(0) = f.Lam[s][0] (rows f.E + 1 = r + 1 elements apart).  No share at a zero column is read: M is 0 at every erased one.
__global__ __launch_bounds__(64) void shamir_erasures_finish_wide_kernel(ShamirFinishWide f, const u64* erased) {
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x;
  WideMont m = f.m;                                // r2 and one in vector registers, as in shamir_correct_finish_wide_kernel
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m.r2[k] = wide_in_vgpr(m.r2[k]);
    m.one[k] = wide_in_vgpr(m.one[k]);
  }
  const u32 count = f.count, words = (count + 63) / 64;
  const u32 L = f.L[s];
  const u64* Mrow = f.M + s * count * 4;
  const u64* erow = erased + s * words;
  bool decodable = L != PVW_SHAMIR_NO_LOCATOR;
  u32 eps = 0;
  if (decodable) {
    u32 nz = 0;
    for (u32 c0 = 0; c0 < count; c0 += 64) {
      const u32 c = c0 + lane;
      u64 mv[4] = {1, 0, 0, 0};
      if (c < count) wide_ld(Mrow + (size_t)c * 4, mv);
      nz += (u32)__popcll(__ballot(wide_zero(mv)));
      eps += (u32)__popcll(shamir_erased_word(erow, c0 / 64, count));
    }
    decodable = nz == L;
  }
  if (!decodable) {
    if (f.mask)
      for (u32 w = lane; w < words; w += 64) f.mask[s * words + w] = 0;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) f.out[s * 4 + k] = 0;
      if (f.nerr) f.nerr[s] = PVW_SHAMIR_NO_LOCATOR;
    }
    return;
  }
  u32 acc[16];
  wide_acc_zero(acc);
  for (u32 c0 = 0; c0 < count; c0 += 64) {
    const u32 c = c0 + lane;
    const bool live = c < count;
    u64 mv[4] = {1, 0, 0, 0};
    if (live) wide_ld(Mrow + (size_t)c * 4, mv);
    const bool zero = wide_zero(mv);
    const u64 bal = __ballot(zero) & ~shamir_erased_word(erow, c0 / 64, count);
    const bool wrong = (bal >> lane) & 1;
    if (lane == 0 && f.mask) f.mask[s * words + c0 / 64] = bal;
    if (wrong && f.col_err) atomicAdd(&f.col_err[c], 1u);
    if (live && !zero) {
      const u64* sp = f.shares + (s * f.secret_stride + (size_t)c * f.point_stride) * 4;
      const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
      u64 y[4], lw[4];
      wide_reduce_p(w, m, y);
      wide_ld(f.lam + (size_t)c * 4, lw);
      wide_mont_mul(lw, mv, m, lw);
      u32 P[16];
      wide_mul_full(y, lw, P);
      wide_acc_add(acc, P, m);
    }
  }
  u64 v[4];
  wide_redc(acc, m, v);
  wave_add_wide(v, m);
  if (lane == 0) {
    u64 l0[4];
    wide_ld(f.Lam + s * (f.E + 1) * 4, l0);
    wide_mont_inv(l0, m, l0);
    wide_mont_mul(v, l0, m, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) f.out[s * 4 + k] = v[k];
    if (f.nerr) f.nerr[s] = L - eps;
  }
}

// The frame of shamir_erasure_mask_kernel with an inner OR over the num_limbs elements of a share, limb_stride apart: a share is
// erased as soon as one of its limbs is flagged.
__global__ __launch_bounds__(64) void shamir_wide_erasure_mask_kernel(const u32* status, const u64* noise, u32 status_bits,
                                                                      u64 noise_bound, u32 count, u32 wb, size_t secret_stride,
                                                                      size_t point_stride, u32 num_limbs, size_t limb_stride, u64* mask) {
  const u32 lane = threadIdx.x;
  const size_t s = blockIdx.x / wb;
  const u32 words = (count + 63) / 64, w0 = (blockIdx.x % wb) * 64;
  const u32 nw = words - w0 < 64 ? words - w0 : 64;
  u64 mine = 0;
  for (u32 k = 0; k < nw; ++k) {
    const u32 c = (w0 + k) * 64 + lane;
    bool e = false;
    if (c < count) {
      const size_t base = s * secret_stride + (size_t)c * point_stride;
      for (u32 w = 0; w < num_limbs; ++w) {
        const size_t off = base + (size_t)w * limb_stride;
        if (status) e = e || (status[off] & status_bits) != 0;
        if (noise) e = e || noise[off] > noise_bound;
      }
    }
    const u64 bal = __ballot(e);
    if (lane == k) mine = bal;
  }
  if (lane < nw) mask[s * words + w0 + lane] = mine;
}

hipError_t launch_shamir_matmul_masked_wide(const ShamirMaskedMatmulWide& b, hipStream_t s) {
  return launch_secret_groups(shamir_matmul_masked_wide_kernel, b, [&](u32 s0) {
    ShamirMaskedMatmulWide p = b;
    p.A += (size_t)s0 * b.secret_stride * 4;
    p.out += (size_t)s0 * b.T * 4;
    p.erased += (size_t)s0 * b.ewords;
    return p;
  }, s);
}

// r <= 2 PVW_SHAMIR_WIDE_MAX_LOCATOR - 1: Gamma, C and B of one wave take at most r + 3 elements of 32 bytes, 131 136 bytes at
// r = 4095 of the 160 KiB a gfx950 workgroup may take; the limit is raised in init_shamir_attributes, each launch asks for
// what its r takes.
hipError_t launch_shamir_bm_erasures_wide(u64* synd, const u64* erased, const u64* x, u64* psi, u32* L, u32 ns, u32 count, u32 r,
                                          const WideMont& m, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  shamir_bm_erasures_wide_kernel<<<dim3(ns), dim3(64), ((size_t)r + 3) * 32, s>>>(synd, erased, x, psi, L, count, r, m);
  return hipGetLastError();
}

hipError_t launch_shamir_erasures_finish_wide(const ShamirFinishWide& f, const u64* erased, u32 ns, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  shamir_erasures_finish_wide_kernel<<<dim3(ns), dim3(64), 0, s>>>(f, erased);
  return hipGetLastError();
}

hipError_t launch_shamir_wide_erasure_mask(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound, u32 count, u32 ns,
                                           size_t secret_stride, size_t point_stride, u32 num_limbs, size_t limb_stride, u64* mask,
                                           hipStream_t s) {
  if (ns == 0 || count == 0) return hipSuccess;
  const u32 words = (count + 63) / 64, wb = (words + 63) / 64;
  const u32 per = 0x7FFFFFFFu / wb;                                // rows per launch: what the grid's x dimension holds
  for (u32 s0 = 0; s0 < ns; s0 += per) {
    const u32 rows = ns - s0 < per ? ns - s0 : per;
    shamir_wide_erasure_mask_kernel<<<dim3(rows * wb), dim3(64), 0, s>>>(
        status ? status + (size_t)s0 * secret_stride : nullptr, noise ? noise + (size_t)s0 * secret_stride : nullptr, status_bits,
        noise_bound, count, wb, secret_stride, point_stride, num_limbs, limb_stride, mask + (size_t)s0 * words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// E + 1 <= PVW_SHAMIR_WIDE_MAX_LOCATOR: C and B of one wave take 2 (E + 1) 32 bytes, up to 128 KiB of the 160 KiB a gfx950 CU has.
// That is more than the 64 KiB a launch gets without asking: the limit is raised once per device (init_shamir_attributes), and
// each launch asks for what its E takes.
// The kernel of 8.21 keeps Gamma, C and B: at most r + 3 elements with r <= 2 PVW_SHAMIR_WIDE_MAX_LOCATOR - 1 = 4095, 131 136 bytes.
hipError_t init_shamir_attributes() {
  hipError_t e = hipFuncSetAttribute((const void*)shamir_bm_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     2 * PVW_SHAMIR_WIDE_MAX_LOCATOR * 32);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)shamir_bm_erasures_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (2 * PVW_SHAMIR_WIDE_MAX_LOCATOR - 1 + 3) * 32);
}
hipError_t launch_shamir_bm_wide(const u64* synd, u64* lam, u32* L, u32 ns, u32 r, const WideMont& m, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  const u32 E = r / 2;
  shamir_bm_wide_kernel<<<dim3(ns), dim3(64), (size_t)2 * (E + 1) * 32, s>>>(synd, lam, L, r, E, m);
  return hipGetLastError();
}

hipError_t launch_shamir_correct_finish_wide(const ShamirFinishWide& f, u32 ns, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  shamir_correct_finish_wide_kernel<<<dim3(ns), dim3(64), 0, s>>>(f);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ evaluation below 2^256
// The table of 8.13 with elements of four words, behind the decode of 8.20 or 8.21, Psi_s standing for Lambda_s.  Forms:
//   xt, scale, C, Xt, Xd                                 public, stored times R
//   shares, YM = REDC(y (M R)), raw = YM x C             plain
//   Psi(x*) = Psi x Xt, Psi'(x*) = Psi x Xd              times R, like M
//   values                                               plain: REDC(raw (scale R)), then REDC with (den R)^-1 R (wide_mont_inv)

// the product of the lanes' values (each times R and below p), the same in every lane: 8 32-bit shuffles a step, no LDS
__device__ __forceinline__ void wave_mul_wide(u64 (&v)[4], const WideMont& m) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    u64 f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = (u64)__shfl_xor((unsigned long long)v[k], off);
    wide_mont_mul(v, f, m, v);
  }
}

// shamir_target_scale_kernel over four words: one wave per target j
__global__ __launch_bounds__(256) void shamir_target_scale_wide_kernel(const u64* x, const u64* xt, u64* scale, u32* coin, u32 count, u32 Tg,
                                                                       WideMont m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 j = blockIdx.x * SH_WAVES + wave;
  if (j >= Tg) return;                                           // wave-uniform
  u64 xs[4], prod[4];
  wide_ld(xt + (size_t)j * 4, xs);
#pragma unroll
  for (int k = 0; k < 4; ++k) prod[k] = m.one[k];
  u32 hit = PVW_SHAMIR_NO_COLUMN;
  for (u32 i = lane; i < count; i += 64) {
    u64 xi[4], d[4];
    wide_ld(x + (size_t)i * 4, xi);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = xs[k];
    wide_sub_p(d, xi, m);
    if (wide_zero(d)) hit = i;
    else wide_mont_mul(prod, d, m, prod);
  }
  wave_mul_wide(prod, m);
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)hit, off);
    hit = o < hit ? o : hit;
  }
  if (lane == 0) {
    wide_st(scale + (size_t)j * 4, prod);
    coin[j] = hit;
  }
}

// C[i][j] = u_i / (x*_j - x_i), 0 where the points coincide.  The shape of shamir_weights_wide_kernel: one thread per target and
// group of SHW_WG columns, the target fastest (thread e = group * Tg + j), so lanes store along a row of C.  The group's
// differences share one inversion, their running products going through the entries' own slots of C; a zero difference enters
// the products as 1, which leaves its slot equal to the one before it.
__global__ __launch_bounds__(256) void shamir_cauchy_wide_kernel(const u64* x, const u64* aux, const u64* xt, u64* C, u32 count, u32 Tg,
                                                                 WideMont m) {
  const size_t groups = ((size_t)count + SHW_WG - 1) / SHW_WG;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= groups * Tg) return;
  const size_t j = e % Tg, i0 = (e / Tg) * SHW_WG;
  const u32 cnt = (size_t)count - i0 < SHW_WG ? (u32)((size_t)count - i0) : SHW_WG;
  u64 xs[4], run[4];
  wide_ld(xt + j * 4, xs);
#pragma unroll
  for (int k = 0; k < 4; ++k) run[k] = m.one[k];
  for (u32 k = 0; k < cnt; ++k) {
    u64 xi[4], d[4];
    wide_ld(x + (i0 + k) * 4, xi);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = xs[i];
    wide_sub_p(d, xi, m);
    if (!wide_zero(d)) wide_mont_mul(run, d, m, run);
    wide_st(C + ((i0 + k) * Tg + j) * 4, run);
  }
  u64 inv[4];
  wide_mont_inv(run, m, inv);
  // back: inv = (d_0 ... d_k)^-1 on entry to step k; d_k^-1 = inv * slot[k-1]
  for (u32 k = cnt; k-- > 0;) {
    u64 xi[4], d[4], pre[4], v[4] = {0, 0, 0, 0};
    wide_ld(x + (i0 + k) * 4, xi);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = xs[i];
    wide_sub_p(d, xi, m);
    if (!wide_zero(d)) {
      if (k) wide_ld(C + ((i0 + k - 1) * Tg + j) * 4, pre);
      else {
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i] = m.one[i];
      }
      u64 u[4];
      wide_mont_mul(inv, pre, m, v);                             // d_k^-1
      wide_mont_mul(inv, d, m, inv);
      wide_ld(aux + (i0 + k) * 4, u);
      wide_mont_mul(v, u, m, v);
    }
    wide_st(C + ((i0 + k) * Tg + j) * 4, v);
  }
}

// Xd[k][j] = k x_j^(k-1) (row 0 is 0), in the frame of shamir_powers_wide_kernel; k R goes along by additions of R
__global__ __launch_bounds__(256) void shamir_dpowers_wide_kernel(const u64* x, u64* X, u32 count, u32 nk, WideMont m) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const u32 k0 = blockIdx.y * 64, k1 = k0 + 64 < nk ? k0 + 64 : nk;
  u64 xc[4], v[4], kr[4];
  wide_ld(x + (size_t)c * 4, xc);
  wide_mont_pow(xc, k0 > 1 ? k0 - 1 : 0, m, v);                  // x_c^(k-1) of the first k >= 1
  const u64 kw[4] = {k0, 0, 0, 0};
  wide_mont_in(kw, m, kr);
  for (u32 k = k0; k < k1; ++k) {
    u64 o[4] = {0, 0, 0, 0};
    if (k) {
      wide_mont_mul(kr, v, m, o);
      wide_mont_mul(v, xc, m, v);
    }
    wide_st(X + ((size_t)k * count + c) * 4, o);
    wide_add_p(kr, m.one, m);
  }
}

// YM[s][c] = y[s][c] M[s][c], plain: one REDC of the share's words times M R.  One thread per element, the column fastest; where
// M is 0 nothing is loaded from the shares, so the words at a wrong or an erased position never enter.
__global__ __launch_bounds__(256) void shamir_ym_wide_kernel(const u64* shares, size_t secret_stride, size_t point_stride, const u64* M,
                                                             u64* YM, u32 ns, u32 count, WideMont m) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)ns * count) return;
  const size_t s = e / count, c = e % count;
  u64 mv[4], v[4] = {0, 0, 0, 0};
  wide_ld(M + e * 4, mv);
  if (!wide_zero(mv)) {
    const u64* sp = shares + (s * secret_stride + c * point_stride) * 4;
    const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
    wide_mont_mul(w, mv, m, v);
  }
  wide_st(YM + e * 4, v);
}

// shamir_evaluate_finish_kernel over four words: one thread per (s, j), the target fastest.  The zero test on M is on the times-R
// form, exact since M < p.
__global__ __launch_bounds__(256) void shamir_evaluate_finish_wide_kernel(ShamirEvalFinishWide f) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)f.ns * f.Tg) return;
  const size_t s = e / f.Tg, j = e % f.Tg;
  const WideMont m = f.m;
  u64 v[4] = {0, 0, 0, 0};
  if (f.nerr[s] != PVW_SHAMIR_NO_LOCATOR) {
    const u32 c = f.coin[j];
    u64 mv[4] = {0, 0, 0, 0};
    if (c != PVW_SHAMIR_NO_COLUMN) wide_ld(f.M + (s * f.count + c) * 4, mv);
    if (!wide_zero(mv)) {
      const u64* sp = f.shares + (s * f.secret_stride + (size_t)c * f.point_stride) * 4;
      const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
      wide_reduce_p(w, m, v);
    } else {
      u64 den[4], sc[4];
      wide_ld((c != PVW_SHAMIR_NO_COLUMN ? f.PsiD : f.PsiT) + e * 4, den);
      wide_ld(f.raw + e * 4, v);
      wide_ld(f.scale + j * 4, sc);
      wide_mont_mul(v, sc, m, v);
      wide_mont_inv(den, m, den);
      wide_mont_mul(v, den, m, v);
    }
  }
  u64* out = f.values + (s * f.value_stride + j) * 4;              // the caller's buffer: word stores
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = v[k];
}

hipError_t launch_shamir_evaluate_weights_wide(const u64* x, const u64* aux, u64* ws, size_t count, u32 nk, size_t Tg, const WideMont& m,
                                               hipStream_t s) {
  const u32 n = (u32)count, tg = (u32)Tg;
  const u64* xt = ws;
  u64 *scale = ws + Tg * 4, *C = scale + Tg * 4, *Xt = C + count * Tg * 4, *Xd = Xt + (size_t)nk * Tg * 4;
  u32* coin = (u32*)(Xd + (size_t)nk * Tg * 4);
  shamir_target_scale_wide_kernel<<<dim3((tg + SH_WAVES - 1) / SH_WAVES), dim3(256), 0, s>>>(x, xt, scale, coin, n, tg, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t threads = ((count + SHW_WG - 1) / SHW_WG) * Tg;
  shamir_cauchy_wide_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(x, aux, xt, C, n, tg, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const dim3 grid((tg + 255) / 256, (nk + 63) / 64);
  shamir_powers_wide_kernel<<<grid, dim3(256), 0, s>>>(xt, Xt, tg, nk, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  shamir_dpowers_wide_kernel<<<grid, dim3(256), 0, s>>>(xt, Xd, tg, nk, m);
  return hipGetLastError();
}

hipError_t launch_shamir_ym_wide(const u64* shares, size_t secret_stride, size_t point_stride, const u64* M, u64* YM, u32 ns, u32 count,
                                 const WideMont& m, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  const size_t blocks = ((size_t)ns * count + 255) / 256;
  shamir_ym_wide_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(shares, secret_stride, point_stride, M, YM, ns, count, m);
  return hipGetLastError();
}

hipError_t launch_shamir_evaluate_finish_wide(const ShamirEvalFinishWide& f, hipStream_t s) {
  if (f.ns == 0 || f.Tg == 0) return hipSuccess;
  const size_t blocks = ((size_t)f.ns * f.Tg + 255) / 256;
  shamir_evaluate_finish_wide_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(f);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ packed shares over a prime below 2^256
// f_d(x) = sum_{j<K} s_{d,j} L_j(x) + Z(x) R_d(x) with R_d = a_{d,1} + ... + a_{d,t} x^(t-1): the frame of shamir_eval_wide_kernel
// (its grid, 256 parties per workgroup, LDS chunks of SHW_JC terms, limb epilogue) as a text of its own at the END of this file,
// so that the kernel of 8.18 and everything behind it keep their code and their place in the code object (8.23 says what a
// shared template body measured).  The Horner loop runs over a_t .. a_1 alone (no e = 0 term) and leaves R_d(x), shifted back to
// a plain value below p.  The K secrets are staged in LDS like coefficients, 256 per chunk, but plain and below p; each is
// multiplied with the lane's Lw[j][party] (stored times 2^256) by wide_mul_full and added by wide_acc_add into ONE unreduced
// accumulator below p 2^256 (the invariant of shamir_tile_product_wide), which starts as R_d(x) zt[party]; SHW_PF weights are in
// flight ahead of their products.  ONE wide_redc gives the share.
#define SHW_PF 4     // weights loaded ahead of their products

// grid and block of shamir_eval_wide_kernel
__global__ __launch_bounds__(256) void shamir_eval_packed_wide_kernel(ShamirWidePackedBatch args) {
  const ShamirWideBatch& b = args.b;
  __shared__ u64 coef[SHW_JC][4];                  // 8 KiB: the chunk's coefficients, scaled, below pn
  __shared__ u32 keyw[8];
  const u32 tid = threadIdx.x;
  const WideMod m = b.m;
  const u32 t = b.degree, nt = t;                  // a_t .. a_1: the secrets come through the weights
  const u32 dx = blockIdx.y, d = b.d_lo + dx;
  const u32 col = blockIdx.x * 256 + tid;
  const u32 party = b.party_lo + col;
  const bool live = col < b.party_hi - b.party_lo;
  const bool drawn = b.coeffs == nullptr && t != 0;
  if (drawn && tid == 0) {
    ChaChaKey k;
    if (b.rnd) k = call_seed(b.rnd->seed, b.rnd->counter + b.rnd_off + (u64)dx * b.key_stride);   // derived when the kernel runs
    else k = b.key[dx];
#pragma unroll
    for (int i = 0; i < 8; ++i) keyw[i] = k.w[i];
  }
  __syncthreads();
  const u32 x = live ? party + 1 : 1;              // x <= n < 2^32
  u64 acc[4] = {0, 0, 0, 0};
  const u32 nchunks = (nt + SHW_JC - 1) / SHW_JC;
  for (u32 c = 0; c < nchunks; ++c) {
    // ---- staging: slot tid holds term e = t - c * SHW_JC - tid, the terms in the order Horner takes them ----
    const u32 first = c * SHW_JC;                  // terms taken before this chunk
    u64 a[4] = {0, 0, 0, 0};
    if (first + tid < nt) {
      const u32 e = t - first - tid;               // 1 .. t
      if (drawn) {
        ChaChaKey k;
#pragma unroll
        for (int i = 0; i < 8; ++i) k.w[i] = keyw[i];
        wide_draw_scaled(k, DOM_SHAMIR, e, m, a);
      } else {
        wide_reduce_scaled(b.coeffs + ((size_t)d * t + (e - 1)) * 4, m, a);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) coef[tid][i] = a[i];
    __syncthreads();
    const u32 cnt = nt - first < SHW_JC ? nt - first : SHW_JC;
    for (u32 jj = 0; jj < cnt; ++jj) {
      u64 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = coef[jj][i];
      wide_step(acc, x, v, m);
    }
    __syncthreads();
  }
  {
    const WideMont mm = args.mm;
    const u32 K = args.pack, cols = b.party_hi - b.party_lo;
    const u32 lc = live ? col : 0;                 // a lane past the range walks column 0 and stores nothing
    wide_shr(acc, m.shift);                        // R_d(x), plain and below p
    u32 T[16], P[16];
    {
      u64 z[4];
      wide_ld(args.zt + (size_t)lc * 4, z);
      wide_mul_full(acc, z, T);                    // acc < p, z < 2^256: below p 2^256
    }
    for (u32 c0 = 0; c0 < K; c0 += SHW_JC) {
      u64 a[4] = {0, 0, 0, 0};
      if (c0 + tid < K) {
        wide_reduce_scaled(b.secrets + ((size_t)d * K + c0 + tid) * 4, m, a);
        wide_shr(a, m.shift);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) coef[tid][i] = a[i];
      __syncthreads();
      const u32 cnt = K - c0 < SHW_JC ? K - c0 : SHW_JC;
      const u64* lw = args.Lw + ((size_t)c0 * cols + lc) * 4;
      for (u32 j0 = 0; j0 < cnt; j0 += SHW_PF) {
        u64 w[SHW_PF][4];
#pragma unroll
        for (u32 q = 0; q < SHW_PF; ++q) {
          const u32 jj = j0 + q < cnt ? j0 + q : cnt - 1;
          wide_ld(lw + (size_t)jj * cols * 4, w[q]);
        }
#pragma unroll
        for (u32 q = 0; q < SHW_PF; ++q) {
          if (j0 + q < cnt) {                      // uniform
            u64 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = coef[j0 + q][i];
            wide_mul_full(v, w[q], P);             // v < p, w < 2^256
            wide_acc_add(T, P, mm);
          }
        }
      }
      __syncthreads();
    }
    wide_redc(T, mm, acc);                         // the share, below p
  }
  if (!live) return;
  if (b.num_limbs == 0) {
    u64* o = b.out + ((size_t)d * b.row_stride + party) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = acc[i];
    return;
  }
  const u64 mask = ((u64)1 << b.limb_bits) - 1;
  for (u32 w = 0; w < b.num_limbs; ++w) {
    const u64 v = (u64)d * b.num_limbs + w;
    if (v >= b.v0 && v < (u64)b.v0 + b.nv) b.out[(size_t)(v - b.v0) * b.row_stride + party] = acc[0] & mask;
    wide_shr(acc, b.limb_bits);                    // limb_bits < 64
  }
}

hipError_t launch_shamir_eval_packed_wide(const ShamirWidePackedBatch& a, hipStream_t s) {
  const ShamirWideBatch& b = a.b;
  if (b.nd == 0 || b.party_hi <= b.party_lo || a.pack == 0) return hipSuccess;
  shamir_eval_packed_wide_kernel<<<dim3((b.party_hi - b.party_lo + 255) / 256, b.nd), dim3(256), 0, s>>>(a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ the weights of packed wide shares
// shamir_packed_basis_kernel and shamir_packed_weights_kernel with elements of four words.  Everything stored is in Montgomery
// form (times R = 2^256), as 8.19 stores its weights.  One lane walks the factorials and makes the ONE inversion, of (K-1)!; the
// workgroup then forms w_j = (-1)^j / (j! (K-1-j)!) and stores w_j R^3: a column's entry is suffix x prefix, two plain values
// below p, so REDC(REDC(suffix prefix) w_j R^3) = suffix prefix w_j R is the entry at the cost of one wide_mul.  The factors
// x + m <= n + K - 1 < 2^32 go into suffix and prefix by wide_step.
__global__ __launch_bounds__(256) void shamir_packed_wide_basis_kernel(u64* w3, u64* invf, u32 K, WideMont mm) {
  if (threadIdx.x == 0) {
    u64 f[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = mm.one[i];
    for (u32 j = 2; j < K; ++j) {                                   // (K-1)! R, K - 1 < p
      const u64 jj[4] = {j, 0, 0, 0};
      wide_mul(jj, f, mm, f);                                       // j (f R) mod p: stays in Montgomery form
    }
    u64 inv[4];
    wide_mont_inv(f, mm, inv);
    for (u32 j = K - 1;; --j) {
      wide_st(invf + (size_t)j * 4, inv);                           // R / j!
      if (j == 0) break;
      const u64 jj[4] = {j, 0, 0, 0};
      wide_mul(jj, inv, mm, inv);
    }
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < K; j += 256) {
    u64 a[4], c[4];
    wide_ld(invf + (size_t)j * 4, a);
    wide_ld(invf + (size_t)(K - 1 - j) * 4, c);
    wide_mont_mul(a, c, mm, a);                                     // R / (j! (K-1-j)!), never 0
    if (j & 1) {
      u64 z[4] = {0, 0, 0, 0};
      wide_sub_p(z, a, mm);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = z[i];
    }
    wide_mont_mul(a, mm.r2, mm, a);                                 // w_j R^2
    wide_mont_mul(a, mm.r2, mm, a);                                 // w_j R^3
    wide_st(w3 + (size_t)j * 4, a);
  }
}

// one thread per column i (x = party_lo + i + 1), lanes store along the rows of Lw: a suffix pass leaves prod_{m>j}(x + m), scaled
// (pvw_wide.h), in Lw[j][i] and ends on Z(x) in full; a prefix pass multiplies prod_{m<j}(x + m) and w_j in
__global__ __launch_bounds__(256) void shamir_packed_wide_weights_kernel(u64* Lw, u64* zt, const u64* w3, u32 K, u32 party_lo, u32 cols,
                                                                         WideMod m, WideMont mm) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cols) return;
  const u32 x = party_lo + i + 1;                                   // x + K - 1 < 2^32
  const u64 zero[4] = {0, 0, 0, 0};
  u64 suf[4] = {1, 0, 0, 0};
  wide_shl(suf, m.shift);
  for (u32 j = K; j-- > 0;) {
    wide_st(Lw + ((size_t)j * cols + i) * 4, suf);
    wide_step(suf, x + j, zero, m);
  }
  wide_shr(suf, m.shift);                                           // Z(x) = x (x + 1) ... (x + K - 1) mod p
  wide_mont_in(suf, mm, suf);
  wide_st(zt + (size_t)i * 4, suf);
  u64 pre[4] = {1, 0, 0, 0};
  wide_shl(pre, m.shift);
  for (u32 j = 0; j < K; ++j) {
    u64* e = Lw + ((size_t)j * cols + i) * 4;
    u64 sv[4], pv[4], wj[4];
    wide_ld(e, sv);
    wide_shr(sv, m.shift);
#pragma unroll
    for (int k = 0; k < 4; ++k) pv[k] = pre[k];
    wide_shr(pv, m.shift);
    wide_ld(w3 + (size_t)j * 4, wj);
    wide_mont_mul(sv, pv, mm, sv);                                  // suffix prefix / R
    wide_mont_mul(sv, wj, mm, sv);                                  // L_j(x) R
    wide_st(e, sv);
    wide_step(pre, x + j, zero, m);
  }
}

// ws: shamir_packed_wide_words
hipError_t launch_shamir_packed_wide_weights(u64* ws, u32 pack, u32 party_lo, u32 party_hi, const WideMod& m, const WideMont& mm,
                                             hipStream_t s) {
  if (pack == 0 || party_hi <= party_lo) return hipSuccess;
  const u32 cols = party_hi - party_lo;
  u64 *Lw = ws, *zt = Lw + (size_t)pack * cols * 4, *w3 = zt + (size_t)cols * 4, *invf = w3 + (size_t)pack * 4;
  shamir_packed_wide_basis_kernel<<<dim3(1), dim3(256), 0, s>>>(w3, invf, pack, mm);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  shamir_packed_wide_weights_kernel<<<dim3((cols + 255) / 256), dim3(256), 0, s>>>(Lw, zt, w3, pack, party_lo, cols, m, mm);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ handover over a prime below 2^256
// The public arithmetic either side of one ct_lincomb_many pass.  A Lagrange weight of 256 bits cannot multiply a ciphertext
// (int64 weights, and the noise would grow by 2^255), but its signed digits of b <= 64 bits can: row m V + v of the weight
// matrix holds digit v of mu_{d,w} = lambda_{d,m} 2^(limb_bits w) mod p at column d NL + w, the combined ciphertext of that row
// decrypts to P_v = sum_{d,w} c_{d,w,v} limb_{d,w}, and sum_v P_v B^v mod p is the new share.  These kernels stand at the END of
// the file, like those of 8.23: nothing before them moves in the code object.  The cut itself is wide_signed_digits (pvw_wide.h).

// x[i] = pt[i] R mod p for target points below p that travel as kernel arguments (shamir_points_wide_kernel takes indices)
__global__ __launch_bounds__(PVW_SHAMIR_WIDE_POINTS) void shamir_points_from_wide_kernel(ShamirWidePoints a, WideMont m) {
  if (threadIdx.x >= a.n) return;
  const u64 x[4] = {a.pt[threadIdx.x][0], a.pt[threadIdx.x][1], a.pt[threadIdx.x][2], a.pt[threadIdx.x][3]};
  u64 xm[4];
  wide_mont_in(x, m, xm);
  wide_st(a.x + (size_t)threadIdx.x * 4, xm);
}
hipError_t launch_shamir_points_from_wide(const u64* points, size_t count, u64* x, const WideMont& m, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += PVW_SHAMIR_WIDE_POINTS) {
    ShamirWidePoints a;
    a.n = (u32)(count - i0 < PVW_SHAMIR_WIDE_POINTS ? count - i0 : PVW_SHAMIR_WIDE_POINTS);
    for (u32 i = 0; i < PVW_SHAMIR_WIDE_POINTS; ++i)
      for (int k = 0; k < 4; ++k) a.pt[i][k] = i < a.n ? points[(i0 + i) * 4 + k] : 0;
    a.x = x + i0 * 4;
    shamir_points_from_wide_kernel<<<dim3(1), dim3(PVW_SHAMIR_WIDE_POINTS), 0, s>>>(a, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// col[i] = the holder that valid holder i is, from kernel arguments like the points (the compaction is the host's)
__global__ __launch_bounds__(PVW_SHAMIR_POINTS) void shamir_handover_columns_kernel(ShamirPoints a) {
  if (threadIdx.x < a.n) ((u32*)a.x)[threadIdx.x] = (u32)a.index[threadIdx.x];
}
hipError_t launch_shamir_handover_columns(const u32* col, size_t count, u32* d_col, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += PVW_SHAMIR_POINTS) {
    ShamirPoints a;
    a.n = (u32)(count - i0 < PVW_SHAMIR_POINTS ? count - i0 : PVW_SHAMIR_POINTS);
    for (u32 i = 0; i < PVW_SHAMIR_POINTS; ++i) a.index[i] = i < a.n ? col[i0 + i] : 0;
    a.x = (u64*)(d_col + i0);                              // i0 is a multiple of 256: aligned
    shamir_handover_columns_kernel<<<dim3(1), dim3(PVW_SHAMIR_POINTS), 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// u_i = (prod_{c != i}(x_i - x_c))^-1 over ALL count columns into aux[0 .. count) (aux[count] = prod_c(-x_c)): the first kernel of
// launch_shamir_correct_weights_wide alone, as it is
hipError_t launch_shamir_column_weights_wide(const u64* x, u64* aux, size_t count, const WideMont& m, hipStream_t s) {
  shamir_prod_wide_kernel<<<dim3((unsigned)((count + 1 + SH_WAVES - 1) / SH_WAVES)), dim3(256), 0, s>>>(x, aux, count, (u32)count - 1, m);
  return hipGetLastError();
}
// scale, coin and C of a group of Tg targets at xt, as they are (the first two launches of launch_shamir_evaluate_weights_wide)
hipError_t launch_shamir_cauchy_wide(const u64* x, const u64* aux, const u64* xt, u64* scale, u64* C, u32* coin, size_t count, size_t Tg,
                                     const WideMont& m, hipStream_t s) {
  const u32 n = (u32)count, tg = (u32)Tg;
  shamir_target_scale_wide_kernel<<<dim3((tg + SH_WAVES - 1) / SH_WAVES), dim3(256), 0, s>>>(x, xt, scale, coin, n, tg, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t threads = ((count + SHW_WG - 1) / SHW_WG) * Tg;
  shamir_cauchy_wide_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(x, aux, xt, C, n, tg, m);
  return hipGetLastError();
}

// One thread per (valid holder i, target j), the holder fastest: the lanes of a wave store along a weight row, NL words apart.
// lambda = scale_j C[i][j] (times R); where the target is a valid holder's point the row is that holder's unit vector, said
// explicitly: scale_j C[i][j] is not 0 at the other columns there.  mu_w = lambda 2^(limb_bits w) is carried along in Montgomery
// form by one product per limb, left, centred and cut.  The matrix is zeroed before the launch: masked holders' columns stay 0.
__global__ __launch_bounds__(256) void shamir_handover_digits_wide_kernel(ShamirHandoverDigits a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.nv * a.Tg) return;
  const u32 i = (u32)(e % a.nv), j = (u32)(e / a.nv);
  const WideMont m = a.m;
  u64 mu[4] = {0, 0, 0, 0};
  const u32 c = a.coin[j];
  if (c != PVW_SHAMIR_NO_COLUMN) {
    if (c == i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) mu[k] = m.one[k];
    }
  } else {
    u64 sc[4], cv[4];
    wide_ld(a.scale + (size_t)j * 4, sc);
    wide_ld(a.C + ((size_t)i * a.Tg + j) * 4, cv);
    wide_mont_mul(sc, cv, m, mu);
  }
  u64 tw[4] = {(u64)1 << a.limb_bits, 0, 0, 0};                    // limb_bits <= 62
  wide_mont_in(tw, m, tw);
  i64* out = a.weights + (size_t)j * a.V * a.ld + (size_t)a.col[i] * a.NL;
  for (u32 w = 0; w < a.NL; ++w) {
    u64 pl[4];
    wide_mont_out(mu, m, pl);
    wide_signed_digits(pl, m.p, a.digit_bits, a.V, out + w, a.ld);
    wide_mont_mul(mu, tw, m, mu);
  }
}
hipError_t launch_shamir_handover_digits_wide(const ShamirHandoverDigits& a, hipStream_t s) {
  const size_t threads = (size_t)a.nv * a.Tg;
  if (!threads) return hipSuccess;
  shamir_handover_digits_wide_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(a);
  return hipGetLastError();
}

// digits[i][V] of values[i] mod p, one thread per value: the cut of the kernel above on operands of the caller's
__global__ __launch_bounds__(256) void shamir_signed_digits_wide_kernel(const u64* values, size_t count, u32 b, u32 V, i64* digits,
                                                                        WideMont m) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const u64 w[4] = {values[i * 4], values[i * 4 + 1], values[i * 4 + 2], values[i * 4 + 3]};
  u64 r[4];
  wide_reduce_p(w, m, r);
  wide_signed_digits(r, m.p, b, V, digits + i * V, 1);
}
hipError_t launch_shamir_signed_digits_wide(const u64* values, size_t count, u32 b, u32 V, i64* digits, const WideMont& m, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += (size_t)1 << 30) {
    const size_t cnt = count - i0 < ((size_t)1 << 30) ? count - i0 : (size_t)1 << 30;
    shamir_signed_digits_wide_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s>>>(values + i0 * 4, cnt, b, V, digits + i0 * V, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// out[i] = sum_v +-|P_{i,v}| B^v mod p, one thread per element i = (party, target): Horner from the top digit in the scaled
// form of wide_step, acc <- acc 2^b + r with multipliers below 2^32 (2^31 as often as b takes, then the rest with the addend).
// r is the magnitude's ww words mod p (wide_reduce_p), p - r where the decode said P < 0.  ONE status word: the OR of the V words
// without the sign bit.
#define SHW_DEC_NEGATIVE 2u                          // PVW_DEC_NEGATIVE (pvw_capi.hip asserts it)
__global__ __launch_bounds__(256) void shamir_wide_from_digits_kernel(const u64* wide, const u32* status, size_t count, u32 V, u32 ww, u32 b,
                                                                      u64* out, u32* status_out, WideMod m, WideMont mm) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const u64 zero[4] = {0, 0, 0, 0};
  u64 acc[4] = {0, 0, 0, 0};
  u32 st = 0;
  for (u32 v = V; v-- > 0;) {
    const u64* src = wide + (i * V + v) * ww;
    const u64 mag[4] = {src[0], ww > 1 ? src[1] : 0, ww > 2 ? src[2] : 0, ww > 3 ? src[3] : 0};
    const u32 sv = status[i * V + v];
    st |= sv;
    u64 r[4];
    wide_reduce_p(mag, mm, r);
    if ((sv & SHW_DEC_NEGATIVE) && (r[0] | r[1] | r[2] | r[3])) {
      u64 br = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const u64 s1 = mm.p[k] - r[k], s2 = s1 - br;
        br = (mm.p[k] < r[k]) | (s1 < br);
        r[k] = s2;
      }
    }
    wide_shl(r, m.shift);
    u32 rem = b;
    for (; rem > 31; rem -= 31) wide_step(acc, 1u << 31, zero, m);
    wide_step(acc, 1u << rem, r, m);
  }
  wide_shr(acc, m.shift);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = acc[k];
  status_out[i] = st & ~SHW_DEC_NEGATIVE;
}
hipError_t launch_shamir_wide_from_digits(const u64* wide, const u32* status, size_t count, u32 V, u32 ww, u32 b, u64* out, u32* status_out,
                                          const WideMod& m, const WideMont& mm, hipStream_t s) {
  for (size_t i0 = 0; i0 < count; i0 += (size_t)1 << 30) {
    const size_t cnt = count - i0 < ((size_t)1 << 30) ? count - i0 : (size_t)1 << 30;
    shamir_wide_from_digits_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s>>>(wide + i0 * V * ww, status + i0 * V, cnt, V, ww, b,
                                                                                           out + i0 * 4, status_out + i0, m, mm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ------------------------------------------------------------------------ the secret points of a packed wide sharing
// x[i] = (p - (m0 + i)) R mod p, the point -(m0 + i) at which a packed row keeps secret m0 + i (m = 0 gives 0): wide_mont_in of m,
// then the negation.  One thread per point and no argument array, so a captured call reads no host memory on replay.  At the END
// of the file, like the kernels of 8.23 and 8.24.
__global__ __launch_bounds__(256) void shamir_packed_secret_points_wide_kernel(u64* x, u32 m0, u32 n, WideMont m) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 mw[4] = {(u64)m0 + i, 0, 0, 0};
  u64 mr[4], v[4] = {0, 0, 0, 0};
  wide_mont_in(mw, m, mr);
  wide_sub_p(v, mr, m);
  wide_st(x + (size_t)i * 4, v);
}
hipError_t launch_shamir_packed_secret_points_wide(u32 m0, size_t count, u64* x, const WideMont& m, hipStream_t s) {
  if (count == 0) return hipSuccess;
  shamir_packed_secret_points_wide_kernel<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s>>>(x, m0, (u32)count, m);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ one-word handover weights from a device mask
// The Lagrange weights of the VALID holders at any points, with the mask read when the kernels run: the points of all D holders
// are public and travel as kernel arguments, the mask bytes are device memory.  A masked holder enters every product as the
// factor 1 and has u_i = 0, so its Cauchy entries and its weights are 0 without a branch.  At the END of the file, like the
// kernels of 8.23 - 8.25: nothing before them moves in the code object.

// the mask of the 64 holders from c0 on, wave-uniform (ct_sum_kernel's walk): bit b is holder c0 + b, NULL is everybody.  c0 is
// walked in 64 bits, as there: count may be anything below 2^32, and c0 + 64 must not wrap
__device__ __forceinline__ u64 shamir_valid_ballot(const unsigned char* valid, u64 c0, u32 lane, u32 count) {
  return __builtin_amdgcn_ballot_w64(c0 + lane < count && (!valid || valid[c0 + lane] != 0));
}

// one wave per holder i, in the frame of shamir_prod_kernel: u_i = (prod_{k valid, k != i}(x_i - x_k))^-1, 0 for a masked i.
// A chunk with no valid holder is skipped, and a lane loads its factor's point only where the ballot has its bit.
__global__ __launch_bounds__(256) void shamir_masked_prod_kernel(const u64* x, const unsigned char* valid, u64* aux, u32 count, Mod m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 i = blockIdx.x * SH_WAVES + wave;
  if (i >= count) return;                                          // wave-uniform
  const u64 own = shamir_valid_ballot(valid, i & ~63u, lane, count);
  if (!((own >> (i & 63)) & 1)) {
    if (lane == 0) aux[i] = 0;
    return;
  }
  const u64 xi = x[i];
  u64 prod = 1;
  for (u64 c0 = 0; c0 < count; c0 += 64) {
    const u64 bal = shamir_valid_ballot(valid, c0, lane, count);
    if (!bal) continue;
    const u64 k = c0 + lane;
    if (((bal >> lane) & 1) && k != i) prod = mulmod(prod, submod(xi, x[k], m.q), m);
  }
  prod = wave_mulmod(prod, m);
  if (lane == 0) aux[i] = invmod_dev(prod, m);
}

// shamir_target_scale_kernel over the valid holders only: a masked column is no factor and can never be `coin`
__global__ __launch_bounds__(256) void shamir_masked_target_scale_kernel(const u64* x, const unsigned char* valid, const u64* xt, u64* scale,
                                                                         u32* coin, u32 count, u32 Tg, Mod m) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 j = blockIdx.x * SH_WAVES + wave;
  if (j >= Tg) return;                                             // wave-uniform
  const u64 xs = xt[j];
  u64 prod = 1;
  u32 hit = PVW_SHAMIR_NO_COLUMN;
  for (u64 c0 = 0; c0 < count; c0 += 64) {
    const u64 bal = shamir_valid_ballot(valid, c0, lane, count);
    if (!bal) continue;
    if ((bal >> lane) & 1) {
      const u64 d = submod(xs, x[c0 + lane], m.q);
      if (d == 0) hit = (u32)(c0 + lane);
      else prod = mulmod(prod, d, m);
    }
  }
  prod = wave_mulmod(prod, m);
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)hit, off);
    hit = o < hit ? o : hit;
  }
  if (lane == 0) {
    scale[j] = prod;
    coin[j] = hit;
  }
}

// One thread per (holder i, target j), the holder fastest: the lanes of a wave store along a weight row.  lambda = scale_j
// C[i][j]; where the target is a valid holder's point the row is that holder's unit vector, said explicitly: scale_j C[i][j] is
// not 0 at the other columns there.  Centred in (-p/2, p/2].  Every word of the group's rows is stored.
__global__ __launch_bounds__(256) void shamir_handover_weights_kernel(const u64* scale, const u64* C, const u32* coin, i64* weights,
                                                                      u32 count, u32 Tg, Mod m) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)count * Tg) return;
  const u32 i = (u32)(e % count), j = (u32)(e / count);
  const u32 c = coin[j];
  const u64 lam = c != PVW_SHAMIR_NO_COLUMN ? (c == i ? 1 : 0) : mulmod(scale[j], C[(size_t)i * Tg + j], m);
  weights[e] = lam > m.q / 2 ? -(i64)(m.q - lam) : (i64)lam;
}

// *num = the number of bytes of valid[0 .. count) that are not 0 (NULL: count), one wave
__global__ __launch_bounds__(64) void shamir_valid_count_kernel(const unsigned char* valid, u32 count, u32* num) {
  u32 n = 0;
  for (u64 c0 = 0; c0 < count; c0 += 64) n += (u32)__builtin_popcountll(shamir_valid_ballot(valid, c0, threadIdx.x, count));
  if (threadIdx.x == 0) *num = n;
}

// valid[c] = 1 iff no row r has status & status_bits or noise > noise_bound at r * row_stride + c * col_stride: a lane per
// column walks the rows (either array may be NULL)
__global__ __launch_bounds__(256) void shamir_valid_mask_kernel(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound,
                                                                u32 count, u32 rows, size_t row_stride, size_t col_stride,
                                                                unsigned char* valid) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  bool bad = false;
  for (u32 r = 0; r < rows; ++r) {
    const size_t off = (size_t)r * row_stride + (size_t)c * col_stride;
    if (status) bad = bad || (status[off] & status_bits) != 0;
    if (noise) bad = bad || noise[off] > noise_bound;
  }
  valid[c] = bad ? 0 : 1;
}

hipError_t launch_shamir_masked_column_weights(const u64* x, const unsigned char* valid, u64* aux, u32* count_out, size_t count, const Mod& m,
                                               hipStream_t s) {
  shamir_masked_prod_kernel<<<dim3((unsigned)((count + SH_WAVES - 1) / SH_WAVES)), dim3(256), 0, s>>>(x, valid, aux, (u32)count, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !count_out) return e;
  shamir_valid_count_kernel<<<dim3(1), dim3(64), 0, s>>>(valid, (u32)count, count_out);
  return hipGetLastError();
}
// ws of the group: xt [Tg] (filled by launch_shamir_points) | scale [Tg] | C [count][Tg] | coin [Tg] (u32); the Cauchy entries by
// shamir_cauchy_kernel as it is, over ALL columns (aux is 0 in a masked one)
hipError_t launch_shamir_handover_weights(const u64* x, const u64* aux, const unsigned char* valid, u64* ws, size_t count, size_t Tg,
                                          i64* weights, const Mod& m, hipStream_t s) {
  const u32 n = (u32)count, tg = (u32)Tg;
  const u64* xt = ws;
  u64 *scale = ws + Tg, *C = scale + Tg;
  u32* coin = (u32*)(C + count * Tg);
  shamir_masked_target_scale_kernel<<<dim3((tg + SH_WAVES - 1) / SH_WAVES), dim3(256), 0, s>>>(x, valid, xt, scale, coin, n, tg, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const u32 bx = (tg + 255) / 256;
  for (u32 i0 = 0; i0 < n; i0 += 65535 * SH_CB) {                  // what the grid's y dimension holds
    const u32 cols = n - i0 < 65535 * SH_CB ? n - i0 : 65535 * SH_CB;
    shamir_cauchy_kernel<<<dim3(bx, (cols + SH_CB - 1) / SH_CB), dim3(256), 0, s>>>(x, aux, xt, C, i0, n, tg, m);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const size_t threads = count * Tg;
  shamir_handover_weights_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(scale, C, coin, weights, n, tg, m);
  return hipGetLastError();
}
hipError_t launch_shamir_valid_mask(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound, u32 count, u32 rows,
                                    size_t row_stride, size_t col_stride, unsigned char* valid, u32* num_valid, hipStream_t s) {
  shamir_valid_mask_kernel<<<dim3((count + 255) / 256), dim3(256), 0, s>>>(status, noise, status_bits, noise_bound, count, rows, row_stride,
                                                                          col_stride, valid);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !num_valid) return e;
  shamir_valid_count_kernel<<<dim3(1), dim3(64), 0, s>>>(valid, count, num_valid);
  return hipGetLastError();
}

}  // namespace pvw

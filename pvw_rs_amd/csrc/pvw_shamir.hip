// pvw_shamir.hip -- Shamir shares on gfx950: shares[d][i] = f_d(i + 1) mod p with
// f_d(x) = s_d + a_{d,1} x + ... + a_{d,t} x^t, for every dealer d and every party i of the context's range.
// The reference has no sharing code (its examples fill the share matrix with arbitrary numbers): the contract is this
// library's own and pvw_shamir_shares_host (pvw_capi.hip) is its plain restatement.
//
// Shape.  A lane owns one party (x = i + 1) and SH_DG dealers; the four waves of a workgroup own the same 64 parties and
// dealers and a quarter of the terms j = 1 .. t each.  A wave starts from x^(j0) by square-and-multiply and then keeps
// pw = x^j up to date with ONE full modular multiply per term, shared by its dealers; a_{d,j} pw goes into one lazy
// accumulator per dealer (pvw_arith.h: 4 x v_mad_u64_u32 into independent sums, reduced once at the end).  The four
// partial sums meet in LDS, as mac_rows sums its waves.
// Coefficients are uniform across a wave: each chunk of SH_JC terms per wave is staged in LDS by the whole workgroup and
// read back as broadcasts ([wave][term][dealer], so one term's SH_DG coefficients are one 32-byte read at the same address
// in every lane).  Drawn coefficients are MADE in that staging phase -- one lane per coefficient, one ChaCha8 block per
// try, its words statically indexed -- so nothing but the shares is ever written to memory; every workgroup of a dealer
// group repeats the draw for its 64 parties (about a quarter of the multiply-add work at 64 parties per workgroup).
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

__device__ __forceinline__ u64 powmod_dev(u64 b, u32 e, const Mod& m) {
  u64 r = 1;
  while (e) {
    if (e & 1) r = mulmod(r, b, m);
    b = mulmod(b, b, m);
    e >>= 1;
  }
  return r;
}

// grid: x = blocks of 64 parties of [party_lo, party_hi), y = groups of SH_DG dealers; 256 threads.
__global__ __launch_bounds__(256) void shamir_eval_kernel(ShamirBatch b) {
  __shared__ u64 coef[SH_WAVES][SH_JC][SH_DG];     // 8 KiB: the chunk's coefficients, below p
  __shared__ u64 part[SH_WAVES][SH_DG][64];        // 8 KiB: the waves' partial sums, below p
  __shared__ u32 keyw[SH_DG][8];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Mod m = b.m;
  const u32 t = b.degree;
  const u32 d0 = blockIdx.y * SH_DG;
  const u32 party = b.party_lo + blockIdx.x * 64 + lane;
  const bool live = party < b.party_hi;
  const bool drawn = b.coeffs == nullptr && t != 0;
  const u32 sh = (u32)__clzll((long long)m.q);
  if (drawn && tid < SH_DG && d0 + tid < b.nd) {
    ChaChaKey k;
    if (b.rnd) k = call_seed(b.rnd->seed, b.rnd->counter + b.rnd_off + d0 + tid);   // derived when the kernel runs
    else k = b.key[d0 + tid];
#pragma unroll
    for (int i = 0; i < 8; ++i) keyw[tid][i] = k.w[i];
  }
  // wave w owns terms j = 1 + w * Q + [0, Q), cut off at t; every wave walks the same number of chunks (barriers)
  const u32 Q = (t + SH_WAVES - 1) / SH_WAVES;
  const u32 jw0 = 1 + wave * Q;
  const u32 nchunks = (Q + SH_JC - 1) / SH_JC;
  const u64 x = live ? (u64)party + 1 : 1;         // x <= n < p
  u64 pw = Q && jw0 <= t ? powmod_dev(x, jw0, m) : 0;
  Acc acc[SH_DG];
#pragma unroll
  for (int g = 0; g < SH_DG; ++g) acc_zero(acc[g]);
  __syncthreads();
  for (u32 c = 0; c < nchunks; ++c) {
    // ---- staging: entry e = (wave, term, dealer) of the chunk, one per lane and trip ----
    for (u32 e = tid; e < SH_WAVES * SH_JC * SH_DG; e += 256) {
      const u32 ew = e / (SH_JC * SH_DG), ej = (e / SH_DG) % SH_JC, eg = e % SH_DG;
      const u32 off = c * SH_JC + ej;              // within the wave's range
      const u32 j = 1 + ew * Q + off;
      u64 a = 0;
      if (off < Q && j <= t && d0 + eg < b.nd) {
        if (drawn) {
          ChaChaKey k;
#pragma unroll
          for (int i = 0; i < 8; ++i) k.w[i] = keyw[eg][i];
          a = shamir_draw(k, j, m.q, sh);
        } else {
          a = reduce_word(b.coeffs[(size_t)(d0 + eg) * t + (j - 1)], m);
        }
      }
      coef[ew][ej][eg] = a;
    }
    __syncthreads();
    // ---- this wave's terms of the chunk ----
    const u32 base = c * SH_JC;
    u32 cnt = 0;
    if (base < Q && jw0 + base <= t) {
      cnt = Q - base < SH_JC ? Q - base : SH_JC;
      const u32 left = t - (jw0 + base) + 1;
      cnt = left < cnt ? left : cnt;
    }
    for (u32 jj = 0; jj < cnt; ++jj) {
      u64 a[SH_DG];
#pragma unroll
      for (int g = 0; g < SH_DG; ++g) a[g] = coef[wave][jj][g];
#pragma unroll
      for (int g = 0; g < SH_DG; ++g) acc_mac_dev(acc[g], a[g], pw);
      pw = mulmod(pw, x, m);
    }
    __syncthreads();
  }
#pragma unroll
  for (int g = 0; g < SH_DG; ++g) part[wave][g][lane] = acc_reduce(acc[g], m);
  __syncthreads();
  // thread (g, lane) adds the four partial sums and the secret and stores dealer d0 + g's share of its party
  {
    const u32 g = wave;                            // SH_WAVES == SH_DG
    const u32 d = d0 + g;
    if (live && d < b.nd) {
      u64 s = reduce_word(b.secrets[d], m);
#pragma unroll
      for (int w = 0; w < SH_WAVES; ++w) s = addmod(s, part[w][g][lane], m.q);
      b.shares[(size_t)d * b.row_stride + party] = s;
    }
  }
}
static_assert(SH_WAVES == SH_DG, "the last phase maps one wave to one dealer of the group");

hipError_t launch_shamir_eval(const ShamirBatch& b, hipStream_t s) {
  if (b.nd == 0 || b.party_hi <= b.party_lo) return hipSuccess;
  const dim3 grid((b.party_hi - b.party_lo + 63) / 64, (b.nd + SH_DG - 1) / SH_DG);
  shamir_eval_kernel<<<grid, dim3(256), 0, s>>>(b);
  return hipGetLastError();
}

}  // namespace pvw

// pvw_sum.hip -- the homomorphic sum of dealers' ciphertexts on gfx950: out = sum over the valid dealers d of in_d, word by
// word mod q of the word's limb (the step examples/pvw.rs:138-170 and examples/pvw_valid_dec.rs:150-209 take on decrypted
// shares, taken on the ciphertexts instead).  An HBM-bound stream: every valid dealer's words are read once.
#include <hip/hip_runtime.h>

#include "pvw_arith.h"
#include "pvw_kernels.h"
#include "pvw_dev.h"

namespace pvw {

// One 16-byte item (two words of one limb: l is even) per thread; a wave reads 1 KiB contiguous of one dealer per load.
// The dealers of the workgroup's slice are walked 64 at a time: lane i reads valid[d0 + i] and the ballot is the slice's
// mask, wave-uniform in a scalar register pair.  The set bits are taken U at a time, so U loads of U VALID dealers are in
// flight per wave whatever the mask looks like, and a dealer that is masked out is never addressed.
// Accumulation is lazy: a 64-bit sum and a 32-bit carry count per word, one 128 -> 64 Barrett step at the end
// (any 64-bit input word is accepted; fewer than 2^32 dealers).
template <int U>
__global__ __launch_bounds__(256) void ct_sum_kernel(SumRegion ra, SumRegion rb, const unsigned char* __restrict__ valid, u32 dealers,
                                                     u32 per_slice, const Mod* __restrict__ mods, u32 ell, u32 L,
                                                     u64* __restrict__ partial, u32 accumulate, u32* __restrict__ count) {
  const size_t items_a = ra.items, total = ra.items + rb.items;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const u32 dlo = blockIdx.y * per_slice;
  const u32 dhi = (dealers - dlo) < per_slice ? dealers : dlo + per_slice;
  // the number of dealers summed: one lane of one workgroup (the mask of ALL dealers, whatever the slices are)
  if (count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
    u32 n = 0;
    for (u64 d0 = 0; d0 < dealers; d0 += 64) {
      const bool on = d0 + lane < dealers && (!valid || valid[d0 + lane] != 0);
      n += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(on));
    }
    if (lane == 0) *count = n;
  }
  const bool live = g < total;
  const bool in_a = g < items_a;
  const size_t it = live ? (in_a ? g : g - items_a) : 0;
  const v2u64* src = reinterpret_cast<const v2u64*>(live ? (in_a ? ra.in : rb.in) : ra.in) + it;
  const size_t stride = (in_a ? ra.stride : rb.stride) / 2;      // 16-byte items between dealers
  u64 s0 = 0, s1 = 0;
  u32 c0 = 0, c1 = 0;
  bool on = dlo + lane < dhi && (!valid || valid[dlo + lane] != 0);
  for (u64 d0 = dlo; d0 < dhi; d0 += 64) {
    u64 m = __builtin_amdgcn_ballot_w64(on);
    on = d0 + 64 + lane < dhi && (!valid || valid[d0 + 64 + lane] != 0);   // the next 64 dealers' bytes, under this chunk's loads
    while (m) {
      v2u64 x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = (v2u64){0, 0};
        if (m) {                                                 // wave-uniform
          const u32 b = (u32)__builtin_ctzll(m);
          m &= m - 1;
          if (live) x[u] = __builtin_nontemporal_load(src + (size_t)(d0 + b) * stride);
        }
      }
      __builtin_amdgcn_sched_barrier(0);                         // every load of the group issued before its first add
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u64 t = s0 + x[u].x;
        c0 += t < s0;
        s0 = t;
        t = s1 + x[u].y;
        c1 += t < s1;
        s1 = t;
      }
    }
  }
  if (!live) return;
  const u32 poly = L * ell;
  const Mod mq = mods[(u32)((2 * it) % poly) / ell];
  v2u64 res = (v2u64){reduce128(s0, c0, mq), reduce128(s1, c1, mq)};
  if (partial) {                                                 // split form: the slice's sum, reduced, for ct_sum_finish
    reinterpret_cast<v2u64*>(partial)[(size_t)blockIdx.y * total + g] = res;
    return;
  }
  v2u64* o = reinterpret_cast<v2u64*>(in_a ? ra.out : rb.out) + it;
  if (accumulate) {                                              // out += sum (a later piece of a staged call)
    const v2u64 p = *o;
    res.x = addmod(res.x, reduce_word(p.x, mq), mq.q);
    res.y = addmod(res.y, reduce_word(p.y, mq), mq.q);
  }
  *o = res;
}

// out = sum of the S slice sums (each below q) of the split form
__global__ __launch_bounds__(256) void ct_sum_finish_kernel(const u64* __restrict__ partial, u32 nslices, SumRegion ra, SumRegion rb,
                                                            const Mod* __restrict__ mods, u32 ell, u32 L, u32 accumulate) {
  const size_t items_a = ra.items, total = ra.items + rb.items;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const bool in_a = g < items_a;
  const size_t it = in_a ? g : g - items_a;
  const u64 q = mods[(u32)((2 * it) % (L * ell)) / ell].q;
  const v2u64* p = reinterpret_cast<const v2u64*>(partial) + g;
  v2u64 acc = p[0];
  for (u32 s = 1; s < nslices; ++s) {
    const v2u64 t = p[(size_t)s * total];
    acc.x = addmod(acc.x, t.x, q);
    acc.y = addmod(acc.y, t.y, q);
  }
  v2u64* o = reinterpret_cast<v2u64*>(in_a ? ra.out : rb.out) + it;
  if (accumulate) {
    const Mod mq = mods[(u32)((2 * it) % (L * ell)) / ell];
    const v2u64 t = *o;
    acc.x = addmod(acc.x, reduce_word(t.x, mq), q);
    acc.y = addmod(acc.y, reduce_word(t.y, mq), q);
  }
  *o = acc;
}

// How many slices the dealers are cut into (1 = the unsplit form), from the shape alone.  With fewer than two workgroups
// per CU (256 CUs) the items alone do not fill the chip -- one party's view at n = 4096, k = 256, l = 8, L = 17 is 69
// workgroups -- so the dealers are cut until about four workgroups per CU exist, never into slices of fewer than 8
// dealers (one group of loads), at most PVW_SUM_MAX_SLICES.
u32 ct_sum_slices(size_t items, size_t dealers) {
  if (items == 0 || dealers == 0) return 1;
  const size_t wgs = (items + 255) / 256;
  long ns = PVW_ENV_INT("PVW_SUM_SPLIT", 0);                     // tuning build: forced slice count (1 = unsplit)
  if (ns <= 0) ns = wgs >= 512 ? 1 : (long)((1024 + wgs - 1) / wgs);
  if (ns > PVW_SUM_MAX_SLICES) ns = PVW_SUM_MAX_SLICES;
  while (ns > 1 && dealers / (size_t)ns < 8) --ns;
  return (u32)(ns < 1 ? 1 : ns);
}

hipError_t launch_ct_sum(const SumRegion& a, const SumRegion& b, const unsigned char* valid, size_t dealers, const DevTables& t, u32 L,
                         u32 ell, u64* partial, u32 nslices, bool accumulate, u32* count, hipStream_t s) {
  const size_t total = a.items + b.items;
  if (total == 0 || dealers == 0 || dealers >> 32) return hipErrorInvalidValue;
  const size_t wgs = (total + 255) / 256;
  if (wgs >> 31) return hipErrorInvalidValue;
  const bool deep = PVW_ENV_INT("PVW_SUM_U", 8) == 16;            // tuning build: 16 loads in flight per wave instead of 8
  if (nslices <= 1 || !partial) {
    if (deep)
      ct_sum_kernel<16><<<dim3((u32)wgs, 1), dim3(256), 0, s>>>(a, b, valid, (u32)dealers, (u32)dealers, t.mods, ell, L, nullptr,
                                                                accumulate ? 1u : 0u, count);
    else
      ct_sum_kernel<8><<<dim3((u32)wgs, 1), dim3(256), 0, s>>>(a, b, valid, (u32)dealers, (u32)dealers, t.mods, ell, L, nullptr,
                                                               accumulate ? 1u : 0u, count);
    return hipGetLastError();
  }
  const u32 per = (u32)((dealers + nslices - 1) / nslices);
  const u32 ny = (u32)((dealers + per - 1) / per);               // no empty slice: every partial plane is written
  ct_sum_kernel<8><<<dim3((u32)wgs, ny), dim3(256), 0, s>>>(a, b, valid, (u32)dealers, per, t.mods, ell, L, partial, 0u, count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ct_sum_finish_kernel<<<dim3((u32)wgs), dim3(256), 0, s>>>(partial, ny, a, b, t.mods, ell, L, accumulate ? 1u : 0u);
  return hipGetLastError();
}

// ---- weighted sums: out = sum over the participating dealers d of w_d * in_d, word by word mod q of the word's limb.
// The frame of ct_sum_kernel (regions, items, the 64-dealer walk, U loads in flight, the split form, accumulate); the
// arithmetic is new.  Lane i of a chunk reads valid[d0 + i] and weights[d0 + i]; a dealer PARTICIPATES when it is valid and its
// weight is not 0, the ballot of that is the chunk's mask, and a dealer outside it is never addressed.  The weight of the
// dealer being consumed is wave-uniform: broadcast from the lane that holds it (v_readlane), and every lane forms
// signed_residue(w, q) for its own limb -- the lane's limb is fixed, so Mod is loaded once; |w| < q costs the compare only.
// Accumulation: acc_mac_dev(acc, residue, word), the lazy 160-bit accumulator of mac_rows: the word is ANY 64-bit value, the
// residue is below q < 2^62, fewer than 2^32 dealers; one acc_reduce at the end.
template <int U>
__global__ __launch_bounds__(256) void ct_lincomb_kernel(SumRegion ra, SumRegion rb, const unsigned char* __restrict__ valid,
                                                         const i64* __restrict__ weights, u32 dealers, u32 per_slice,
                                                         const Mod* __restrict__ mods, u32 ell, u32 L, u64* __restrict__ partial,
                                                         u32 accumulate, u32* __restrict__ count) {
  const size_t items_a = ra.items, total = ra.items + rb.items;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const u32 dlo = blockIdx.y * per_slice;
  const u32 dhi = (dealers - dlo) < per_slice ? dealers : dlo + per_slice;
  // the number of participating dealers: one wave of one workgroup (ALL dealers, whatever the slices are)
  if (count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
    u32 n = 0;
    for (u64 d0 = 0; d0 < dealers; d0 += 64) {
      const bool on = d0 + lane < dealers && (!valid || valid[d0 + lane] != 0) && weights[d0 + lane] != 0;
      n += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(on));
    }
    if (lane == 0) *count = n;
  }
  const bool live = g < total;
  const bool in_a = g < items_a;
  const size_t it = live ? (in_a ? g : g - items_a) : 0;
  const v2u64* src = reinterpret_cast<const v2u64*>(live ? (in_a ? ra.in : rb.in) : ra.in) + it;
  const size_t stride = (in_a ? ra.stride : rb.stride) / 2;      // 16-byte items between dealers
  const u32 poly = L * ell;
  const Mod mq = mods[(u32)((2 * it) % poly) / ell];
  Acc a0, a1;
  acc_zero(a0);
  acc_zero(a1);
  // this chunk's weights, one dealer a lane (0 beyond the slice), and its participation bit
  auto weight_of = [&](u64 d) -> i64 { return d < dhi ? weights[d] : 0; };
  auto takes_part = [&](u64 d, i64 w) -> bool { return d < dhi && w != 0 && (!valid || valid[d] != 0); };
  i64 wt = weight_of((u64)dlo + lane);
  bool on = takes_part((u64)dlo + lane, wt);
  for (u64 d0 = dlo; d0 < dhi; d0 += 64) {
    u64 m = __builtin_amdgcn_ballot_w64(on);
    const i64 wcur = wt;
    wt = weight_of(d0 + 64 + lane);                              // the next 64 dealers' bytes and weights, under this chunk's loads
    on = takes_part(d0 + 64 + lane, wt);
    while (m) {
      v2u64 x[U];
      u32 b[U];                                                  // the lane that holds the slot's weight; 64: the slot is unused
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = (v2u64){0, 0};
        b[u] = 64;
        if (m) {                                                 // wave-uniform
          b[u] = (u32)__builtin_ctzll(m);
          m &= m - 1;
          if (live) x[u] = __builtin_nontemporal_load(src + (size_t)(d0 + b[u]) * stride);
        }
      }
      __builtin_amdgcn_sched_barrier(0);                         // every load of the group issued before its first multiply
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)(u64)wcur, (int)(b[u] & 63));
        const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)((u64)wcur >> 32), (int)(b[u] & 63));
        const i64 w = b[u] < 64 ? (i64)(((u64)hi << 32) | lo) : 0;   // wave-uniform; an unused slot of the last group: 0 * 0
        const u64 r = signed_residue(w, mq);
        acc_mac_dev(a0, r, x[u].x);
        acc_mac_dev(a1, r, x[u].y);
      }
    }
  }
  if (!live) return;
  v2u64 res = (v2u64){acc_reduce(a0, mq), acc_reduce(a1, mq)};
  if (partial) {                                                 // split form: the slice's result, reduced, for ct_sum_finish
    reinterpret_cast<v2u64*>(partial)[(size_t)blockIdx.y * total + g] = res;
    return;
  }
  v2u64* o = reinterpret_cast<v2u64*>(in_a ? ra.out : rb.out) + it;
  if (accumulate) {                                              // out += the combination (a later piece of a staged call)
    const v2u64 p = *o;
    res.x = addmod(res.x, reduce_word(p.x, mq), mq.q);
    res.y = addmod(res.y, reduce_word(p.y, mq), mq.q);
  }
  *o = res;
}

hipError_t launch_ct_lincomb(const SumRegion& a, const SumRegion& b, const unsigned char* valid, const i64* weights, size_t dealers,
                             const DevTables& t, u32 L, u32 ell, u64* partial, u32 nslices, bool accumulate, u32* count,
                             hipStream_t s) {
  const size_t total = a.items + b.items;
  if (total == 0 || dealers == 0 || dealers >> 32 || !weights) return hipErrorInvalidValue;
  const size_t wgs = (total + 255) / 256;
  if (wgs >> 31) return hipErrorInvalidValue;
  if (nslices <= 1 || !partial) {
    ct_lincomb_kernel<8><<<dim3((u32)wgs, 1), dim3(256), 0, s>>>(a, b, valid, weights, (u32)dealers, (u32)dealers, t.mods, ell, L,
                                                                 nullptr, accumulate ? 1u : 0u, count);
    return hipGetLastError();
  }
  const u32 per = (u32)((dealers + nslices - 1) / nslices);
  const u32 ny = (u32)((dealers + per - 1) / per);               // no empty slice: every partial plane is written
  ct_lincomb_kernel<8><<<dim3((u32)wgs, ny), dim3(256), 0, s>>>(a, b, valid, weights, (u32)dealers, per, t.mods, ell, L, partial, 0u,
                                                                count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ct_sum_finish_kernel<<<dim3((u32)wgs), dim3(256), 0, s>>>(partial, ny, a, b, t.mods, ell, L, accumulate ? 1u : 0u);
  return hipGetLastError();
}

// ---- many weighted sums of the same dealers: out_r = sum_d w[r][d] * in_d for a tile of RT rows of the weight
// matrix.  The frame of ct_lincomb_kernel; each thread keeps RT accumulator pairs, so a 16-byte item is loaded and addressed
// once and multiply-added RT times.  Lane i of a chunk holds its dealer's RT weights (0 for the rows the ragged last tile does
// not have); a dealer is in the chunk's mask when it is valid and ANY of the tile's weights is not 0, and a zero weight inside
// such a dealer contributes 0 * x.  Row r of the tile is written r * out_stride words behind the region's `out`; the split
// form's planes lie [row][slice][items], so ct_sum_finish_kernel adds up one row's slices as it does for one combination.
template <int RT, int U>
__global__ __launch_bounds__(256) void ct_lincomb_many_kernel(SumRegion ra, SumRegion rb, size_t out_stride_a, size_t out_stride_b,
                                                              const unsigned char* __restrict__ valid, const i64* __restrict__ weights,
                                                              size_t wstride, u32 nrows, u32 dealers, u32 per_slice,
                                                              const Mod* __restrict__ mods, u32 ell, u32 L, u64* __restrict__ partial,
                                                              u32 accumulate, u32* __restrict__ counts) {
  const size_t items_a = ra.items, total = ra.items + rb.items;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const u32 dlo = blockIdx.y * per_slice;
  const u32 dhi = (dealers - dlo) < per_slice ? dealers : dlo + per_slice;
  // each row's number of participating dealers: one wave of one workgroup (ALL dealers, whatever the slices are)
  if (counts && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
    for (u32 r = 0; r < nrows; ++r) {
      u32 n = 0;
      for (u64 d0 = 0; d0 < dealers; d0 += 64) {
        const bool on = d0 + lane < dealers && (!valid || valid[d0 + lane] != 0) && weights[r * wstride + d0 + lane] != 0;
        n += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(on));
      }
      if (lane == 0) counts[r] = n;
    }
  }
  const bool live = g < total;
  const bool in_a = g < items_a;
  const size_t it = live ? (in_a ? g : g - items_a) : 0;
  const v2u64* src = reinterpret_cast<const v2u64*>(live ? (in_a ? ra.in : rb.in) : ra.in) + it;
  const size_t stride = (in_a ? ra.stride : rb.stride) / 2;      // 16-byte items between dealers
  const u32 poly = L * ell;
  const Mod mq = mods[(u32)((2 * it) % poly) / ell];
  Acc a0[RT], a1[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) { acc_zero(a0[r]); acc_zero(a1[r]); }
  // this chunk's weights, RT per lane and dealer (0 beyond the slice and beyond the tile's rows), and the dealer's mask bit
  i64 wt[RT];
  auto load_chunk = [&](u64 d) -> bool {
    bool any = false;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      wt[r] = d < dhi && (u32)r < nrows ? weights[r * wstride + d] : 0;
      any = any || wt[r] != 0;
    }
    return any && (!valid || valid[d] != 0);                     // any: d < dhi
  };
  bool on = load_chunk((u64)dlo + lane);
  for (u64 d0 = dlo; d0 < dhi; d0 += 64) {
    u64 m = __builtin_amdgcn_ballot_w64(on);
    i64 wcur[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) wcur[r] = wt[r];
    on = load_chunk(d0 + 64 + lane);                             // the next 64 dealers' bytes and weights, under this chunk's loads
    while (m) {
      v2u64 x[U];
      u32 b[U];                                                  // the lane that holds the slot's weights; 64: the slot is unused
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = (v2u64){0, 0};
        b[u] = 64;
        if (m) {                                                 // wave-uniform
          b[u] = (u32)__builtin_ctzll(m);
          m &= m - 1;
          if (live) x[u] = __builtin_nontemporal_load(src + (size_t)(d0 + b[u]) * stride);
        }
      }
      __builtin_amdgcn_sched_barrier(0);                         // every load of the group issued before its first multiply
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)(u64)wcur[r], (int)(b[u] & 63));
          const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)((u64)wcur[r] >> 32), (int)(b[u] & 63));
          const i64 w = b[u] < 64 ? (i64)(((u64)hi << 32) | lo) : 0;   // wave-uniform; an unused slot of the last group: 0 * 0
          const u64 res = signed_residue(w, mq);
          acc_mac_dev(a0[r], res, x[u].x);
          acc_mac_dev(a1[r], res, x[u].y);
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    if ((u32)r >= nrows) break;                                  // the ragged last tile: nothing is stored for its empty rows
    v2u64 res = (v2u64){acc_reduce(a0[r], mq), acc_reduce(a1[r], mq)};
    if (partial) {                                               // split form: the slice's result for row r, reduced
      reinterpret_cast<v2u64*>(partial)[((size_t)r * gridDim.y + blockIdx.y) * total + g] = res;
      continue;
    }
    v2u64* o = reinterpret_cast<v2u64*>((in_a ? ra.out : rb.out) + (size_t)r * (in_a ? out_stride_a : out_stride_b)) + it;
    if (accumulate) {                                            // out += the combination (a later piece of a staged call)
      const v2u64 p = *o;
      res.x = addmod(res.x, reduce_word(p.x, mq), mq.q);
      res.y = addmod(res.y, reduce_word(p.y, mq), mq.q);
    }
    *o = res;
  }
}

// The row tile of the many form, from the shape alone (profiles/r13_ct_lincomb_many.txt).  The RT = 2 kernel keeps three
// workgroups a CU resident (768 on the chip), the RT = 4 kernel two: a grid the RT = 2 kernel finishes in one round is fastest
// with it (config-5 shard column, 545 workgroups: 1.40x over single passes against 1.22x), and so is every split form; from
// 768 workgroups on the second round is there anyway and the wider reuse wins (config 3 whole rows, 1156: 1.81x against
// 1.77x; 884: 1.57x against 1.29x).  RT = 8 (one wave a SIMD) loses everywhere and is instantiated for the measurement only.
// Tuning build: PVW_SUM_RT = 2 / 4 / 8 forces the tile.
u32 ct_lincomb_many_tile(size_t items, u32 nslices) {
  const long rt = PVW_ENV_INT("PVW_SUM_RT", 0);
  if (rt == 2 || rt == 4 || rt == 8) return (u32)rt;
  return nslices <= 1 && (items + 255) / 256 >= 768 ? 4u : 2u;
}

template <int RT, int U>
static hipError_t ct_lincomb_many_tile_launch(const SumRegion& a, const SumRegion& b, size_t osa, size_t osb, const unsigned char* valid,
                                              const i64* weights, size_t wstride, u32 nrows, size_t dealers, const DevTables& t, u32 L,
                                              u32 ell, u64* partial, u32 nslices, bool accumulate, u32* counts, hipStream_t s) {
  const size_t total = a.items + b.items;
  const u32 wgs = (u32)((total + 255) / 256);
  if (nslices <= 1 || !partial) {
    ct_lincomb_many_kernel<RT, U><<<dim3(wgs, 1), dim3(256), 0, s>>>(a, b, osa, osb, valid, weights, wstride, nrows, (u32)dealers,
                                                                      (u32)dealers, t.mods, ell, L, nullptr, accumulate ? 1u : 0u, counts);
    return hipGetLastError();
  }
  const u32 per = (u32)((dealers + nslices - 1) / nslices);
  const u32 ny = (u32)((dealers + per - 1) / per);               // no empty slice: every partial plane is written
  ct_lincomb_many_kernel<RT, U><<<dim3(wgs, ny), dim3(256), 0, s>>>(a, b, osa, osb, valid, weights, wstride, nrows, (u32)dealers, per,
                                                                     t.mods, ell, L, partial, 0u, counts);
  hipError_t e = hipGetLastError();
  for (u32 r = 0; r < nrows && e == hipSuccess; ++r) {           // one row's slices: planes r * ny .. r * ny + ny - 1
    SumRegion fa = a, fb = b;
    fa.out = a.out + (size_t)r * osa;
    fb.out = b.out + (size_t)r * osb;
    ct_sum_finish_kernel<<<dim3(wgs), dim3(256), 0, s>>>(partial + (size_t)r * ny * total * 2, ny, fa, fb, t.mods, ell, L,
                                                         accumulate ? 1u : 0u);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_ct_lincomb_many(const SumRegion& a, const SumRegion& b, size_t out_stride_a, size_t out_stride_b,
                                  const unsigned char* valid, const i64* weights, size_t wstride, size_t nrows, size_t dealers,
                                  const DevTables& t, u32 L, u32 ell, u64* partial, u32 nslices, bool accumulate, u32* counts,
                                  hipStream_t s) {
  const size_t total = a.items + b.items;
  if (total == 0 || dealers == 0 || dealers >> 32 || !weights || nrows == 0 || nrows >> 31) return hipErrorInvalidValue;
  if (((total + 255) / 256) >> 31) return hipErrorInvalidValue;
  const u32 tile = ct_lincomb_many_tile(total, partial ? nslices : 1);
  if ((size_t)(nslices > 1 && partial ? nslices : 0) * tile * total > ct_sum_partial_items_max()) return hipErrorInvalidValue;
  // One pass over the dealers per row tile.  The rows a full tile leaves over go to the narrowest kernel that holds them -- a
  // ragged tile pays for its empty rows (R = 2 in an RT = 4 tile: 0.91x of two single passes at config 3) -- down to the
  // single-combination kernel for one row.
  u32 nr = 0;
  for (size_t r0 = 0; r0 < nrows; r0 += nr) {
    const size_t rem = nrows - r0;
    const u32 rt = tile == 8 && rem >= 8 ? 8 : tile >= 4 && rem >= 3 ? 4 : rem >= 2 ? 2 : 1;
    nr = (u32)(rem < rt ? rem : rt);
    SumRegion ta = a, tb = b;
    ta.out = a.out + r0 * out_stride_a;
    tb.out = b.out + r0 * out_stride_b;
    const i64* wr = weights + r0 * wstride;
    u32* cr = counts ? counts + r0 : nullptr;
    hipError_t e;
    if (rt == 1)
      e = launch_ct_lincomb(ta, tb, valid, wr, dealers, t, L, ell, partial, nslices, accumulate, cr, s);
    else if (rt == 2)
      e = ct_lincomb_many_tile_launch<2, 8>(ta, tb, out_stride_a, out_stride_b, valid, wr, wstride, nr, dealers, t, L, ell, partial,
                                            nslices, accumulate, cr, s);
    else if (rt == 4)
      e = ct_lincomb_many_tile_launch<4, 8>(ta, tb, out_stride_a, out_stride_b, valid, wr, wstride, nr, dealers, t, L, ell, partial,
                                            nslices, accumulate, cr, s);
    else
      e = ct_lincomb_many_tile_launch<8, 4>(ta, tb, out_stride_a, out_stride_b, valid, wr, wstride, nr, dealers, t, L, ell, partial,
                                            nslices, accumulate, cr, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// p[0 .. words) = 0 as a kernel on `s`: the clearing of a small key-derived scratch region that has to stay ordered behind its
// last reader when the call is captured into a graph and replayed
__global__ __launch_bounds__(256) void wipe_words_kernel(u64* __restrict__ p, size_t words) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < words) p[i] = 0;
}
hipError_t launch_wipe_words(u64* p, size_t words, hipStream_t s) {
  if (!words) return hipSuccess;
  wipe_words_kernel<<<dim3((u32)((words + 255) / 256)), dim3(256), 0, s>>>(p, words);
  return hipGetLastError();
}

}  // namespace pvw

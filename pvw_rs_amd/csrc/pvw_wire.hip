// pvw_wire.hip -- the version-1 wire format's polynomial codec on gfx950.
//
// A packed polynomial is its L limb rows back to back; row i holds the l residues of limb i at w_i bits each (w_i = bit
// length of q_i), least significant bit first, read as a little-endian byte string.  poly_bytes = (l/8) sum_i w_i.
//
// Unit: G = 128/l polynomials.  Their packed bytes are 16 sum_i w_i -- a whole number of 16-byte chunks -- and their words
// are 128 L u64 (1 KiB per limb), so a unit is staged in LDS whole.  A workgroup takes a run of 16 polynomials (16/G units,
// one after the other); its output starts at 16 poly_bytes times its index, a multiple of 16.
//
//   wire_pack_kernel    words -> LDS (coalesced 16-byte loads, reduced with the limb's Barrett constants) -> one 16-byte
//                       chunk of the packed unit per lane, assembled from the residues it covers -> 16-byte stores.  Only
//                       the last chunk of a count that is not a multiple of G is narrower (byte stores).
//   wire_unpack_kernel  packed chunks -> LDS (coalesced 16-byte loads; the narrower last chunk byte by byte) -> every
//                       residue extracted, compared with q_i -> 16-byte stores of two words.  Rejected residues (>= q_i)
//                       are counted: one atomic add per wave into *bad.  With words == NULL only the count is made.
// Both are memory-bound: every global byte is read or written once, with 16-byte lane accesses.
#include <hip/hip_runtime.h>

#include "pvw_dev.h"
#include "pvw_kernels.h"

namespace pvw {

namespace {
constexpr int WIRE_THREADS = 256;
constexpr int WIRE_RUN = 16;                 // polynomials per workgroup
constexpr u32 WIRE_MAX_L = 64;               // LDS: 1 KiB of words per limb

struct WireLimbs {
  Mod m[WIRE_MAX_L];
  u32 w[WIRE_MAX_L];           // bits per residue
  u32 rowbit[WIRE_MAX_L + 1];  // first bit of row i inside a packed polynomial; rowbit[L] = poly_bits
};

// limb tables into LDS (every thread of the workgroup calls this, then syncs)
__device__ __forceinline__ void wire_limbs(WireLimbs& t, const Mod* __restrict__ mods, u32 L, u32 ell) {
  for (u32 i = threadIdx.x; i < L; i += WIRE_THREADS) {
    const Mod m = mods[i];
    t.m[i] = m;
    t.w[i] = 64u - (u32)__clzll((long long)m.q);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 acc = 0;
    for (u32 i = 0; i < L; ++i) {
      t.rowbit[i] = acc;
      acc += t.w[i] * ell;
    }
    t.rowbit[L] = acc;
  }
  __syncthreads();
}
}  // namespace

__global__ __launch_bounds__(WIRE_THREADS) void wire_pack_kernel(const u64* __restrict__ words, size_t count,
                                                                 unsigned char* __restrict__ out, const Mod* __restrict__ mods,
                                                                 u32 L, u32 ell) {
  __shared__ WireLimbs t;
  extern __shared__ v2u64 wire_lds[];                       // one unit of reduced words: [G][L][ell]
  u64* res = reinterpret_cast<u64*>(wire_lds);
  wire_limbs(t, mods, L, ell);
  const u32 G = 128 / ell;
  const u32 poly_words = L * ell, poly_bits = t.rowbit[L];
  const size_t poly_bytes = poly_bits / 8;
  const size_t p0 = (size_t)blockIdx.x * WIRE_RUN;
  for (u32 u0 = 0; u0 < WIRE_RUN; u0 += G) {
    const size_t pu = p0 + u0;
    if (pu >= count) break;
    const u32 np = (count - pu) < G ? (u32)(count - pu) : G;
    // 1. the unit's words, coalesced, reduced below q_i
    const v2u64* src = reinterpret_cast<const v2u64*>(words + pu * poly_words);
    const u32 pairs = np * poly_words / 2;
    for (u32 x = threadIdx.x; x < pairs; x += WIRE_THREADS) {
      const v2u64 v = __builtin_nontemporal_load(src + x);
      const u32 limb = (2 * x / ell) % L;
      wire_lds[x] = (v2u64){reduce_word(v.x, t.m[limb]), reduce_word(v.y, t.m[limb])};
    }
    __syncthreads();
    // 2. one 16-byte chunk of the packed unit per lane
    const u32 unit_bits = np * poly_bits;
    const u32 chunks = (unit_bits + 127) / 128;
    unsigned char* dst = out + pu * poly_bytes;
    for (u32 c = threadIdx.x; c < chunks; c += WIRE_THREADS) {
      const u32 b = c * 128;
      const u32 want = (unit_bits - b) < 128 ? unit_bits - b : 128;
      u32 g = b / poly_bits, o = b - g * poly_bits, i = 0;
      while (o >= t.rowbit[i + 1]) ++i;
      u32 w = t.w[i];
      u32 j = (o - t.rowbit[i]) / w;
      u32 s = (o - t.rowbit[i]) - j * w;
      u128 acc = 0;
      u32 pos = 0;
      while (pos < want) {
        acc |= (u128)(res[((size_t)g * L + i) * ell + j] >> s) << pos;
        pos += w - s;
        s = 0;
        if (++j == ell) {
          j = 0;
          if (++i == L) { i = 0; ++g; }
          w = t.w[i];
        }
      }
      if (want == 128) {
        reinterpret_cast<v2u64*>(dst)[c] = (v2u64){(u64)acc, (u64)(acc >> 64)};
      } else {                                                // the count's tail: bytes of the last chunk only
        for (u32 y = 0; y < want / 8; ++y) dst[(size_t)c * 16 + y] = (unsigned char)(acc >> (8 * y));
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(WIRE_THREADS) void wire_unpack_kernel(const unsigned char* __restrict__ in, size_t count,
                                                                   u64* __restrict__ words, unsigned long long* __restrict__ bad,
                                                                   const Mod* __restrict__ mods, u32 L, u32 ell) {
  __shared__ WireLimbs t;
  extern __shared__ v2u64 wire_lds[];                       // one unit's packed bytes (+ one zero chunk)
  const u64* pk = reinterpret_cast<const u64*>(wire_lds);
  wire_limbs(t, mods, L, ell);
  const u32 G = 128 / ell;
  const u32 poly_words = L * ell, poly_bits = t.rowbit[L];
  const size_t poly_bytes = poly_bits / 8;
  const size_t p0 = (size_t)blockIdx.x * WIRE_RUN;
  u32 nbad = 0;
  for (u32 u0 = 0; u0 < WIRE_RUN; u0 += G) {
    const size_t pu = p0 + u0;
    if (pu >= count) break;
    const u32 np = (count - pu) < G ? (u32)(count - pu) : G;
    // 1. the unit's packed bytes, 16-byte aligned chunks, coalesced
    const u32 unit_bytes = np * (poly_bits / 8);
    const u32 full = unit_bytes / 16, chunks = (unit_bytes + 15) / 16;
    const unsigned char* src = in + pu * poly_bytes;
    for (u32 c = threadIdx.x; c <= chunks; c += WIRE_THREADS) {
      v2u64 v = (v2u64){0, 0};
      if (c < full) {
        v = __builtin_nontemporal_load(reinterpret_cast<const v2u64*>(src) + c);
      } else if (c < chunks) {                                // the count's tail
        for (u32 y = 0; y < unit_bytes - 16 * c; ++y) {
          const u64 by = src[(size_t)c * 16 + y];
          if (y < 8) v.x |= by << (8 * y);
          else v.y |= by << (8 * (y - 8));
        }
      }
      wire_lds[c] = v;
    }
    __syncthreads();
    // 2. two residues per lane, extracted, checked, stored as one 16-byte access
    v2u64* dst = reinterpret_cast<v2u64*>(words ? words + pu * poly_words : nullptr);
    const u32 pairs = np * poly_words / 2;
    for (u32 x = threadIdx.x; x < pairs; x += WIRE_THREADS) {
      const u32 e = 2 * x, g = e / poly_words, r = e - g * poly_words, i = r / ell, j = r - i * ell;
      const u32 w = t.w[i];
      const u64 q = t.m[i].q, mask = (1ull << w) - 1;
      u64 v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32 o = g * poly_bits + t.rowbit[i] + (j + h) * w;
        const u32 sh = o & 63;
        u64 x0 = pk[o >> 6] >> sh;
        if (sh + w > 64) x0 |= pk[(o >> 6) + 1] << (64 - sh);
        v[h] = x0 & mask;
        nbad += v[h] >= q;
      }
      if (dst) dst[x] = (v2u64){v[0], v[1]};
    }
    __syncthreads();
  }
  // one atomic add per wave
  for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
}

size_t wire_lds_bytes(u32 L) { return (size_t)L * 1024 + 16; }

hipError_t launch_wire_pack(const u64* words, size_t count, unsigned char* out, const Mod* mods, u32 L, u32 ell, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (L == 0 || L > WIRE_MAX_L || ell < 8 || ell > 128 || (ell & (ell - 1))) return hipErrorInvalidValue;
  const size_t blocks = (count + WIRE_RUN - 1) / WIRE_RUN;
  hipLaunchKernelGGL(wire_pack_kernel, dim3((u32)blocks), dim3(WIRE_THREADS), wire_lds_bytes(L), s, words, count, out, mods, L,
                     ell);
  return hipGetLastError();
}

hipError_t launch_wire_unpack(const unsigned char* in, size_t count, u64* words, unsigned long long* bad, const Mod* mods, u32 L,
                              u32 ell, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (L == 0 || L > WIRE_MAX_L || ell < 8 || ell > 128 || (ell & (ell - 1))) return hipErrorInvalidValue;
  const size_t blocks = (count + WIRE_RUN - 1) / WIRE_RUN;
  hipLaunchKernelGGL(wire_unpack_kernel, dim3((u32)blocks), dim3(WIRE_THREADS), wire_lds_bytes(L), s, in, count, words, bad, mods,
                     L, ell);
  return hipGetLastError();
}

hipError_t init_wire_attributes() {
  const int lds = (int)wire_lds_bytes(WIRE_MAX_L);
  hipError_t e = hipFuncSetAttribute((const void*)wire_pack_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)wire_unpack_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

}  // namespace pvw

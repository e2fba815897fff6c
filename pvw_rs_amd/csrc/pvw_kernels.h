// pvw_kernels.h -- launch interface of the gfx950 kernels (pvw_mac / pvw_poly / pvw_decrypt / pvw_decode_kernels / pvw_gemm .hip).
#pragma once
#include <hip/hip_runtime.h>

#include "pvw_arith.h"
#include "pvw_chacha.h"
#include "pvw_decode.h"
#include "pvw_wide.h"

// PVW_TUNING selects the MEASUREMENT build (libpvw_hip_tuning.so, pvw_rs_amd/build.py): only there are the
// timing switches (PVW_DECODE_TIMING, PVW_GEMM_ZERO_OPERANDS), the schedule selectors (PVW_MAC_VARIANT, PVW_MAC_PACKED,
// PVW_DEC_C, PVW_DECODE_VARIANT, ...) and the read-bandwidth probe compiled in.  The shipped library (PVW_TUNING 0) holds the
// shape-selected schedules only and reads NO environment variable: nothing outside the arguments of a call can
// change what it computes (the reference samples unconditionally, src/crypto/encryption.rs:135-167).
#ifndef PVW_TUNING
#define PVW_TUNING 0
#endif
#if PVW_TUNING
#include <cstdlib>
#define PVW_ENV_INT(name, dflt) ([]() -> long { const char* e_ = getenv(name); return e_ ? atol(e_) : (long)(dflt); }())
#else
#define PVW_ENV_INT(name, dflt) ((long)(dflt))
#endif

namespace pvw {

enum { DOM_R = 0, DOM_E1 = 1, DOM_E2 = 2, DOM_SK = 3, DOM_EKEY = 4, DOM_CRS = 5, DOM_GAUSS = 6, DOM_PK = 7, DOM_CALL = 8 };

// Device randomness state of pvw_rnd_state: the 32-byte seed S and the counter c of the next call.  An encrypt that reads
// it seeds dealer / call i with call_seed(S, c + i) when its kernels RUN (not when they are enqueued), so graph replays and
// queued eager calls each draw fresh randomness.  `base` is the counter the running call started from: every prologue that
// reads the state copies `counter` there (one lane), later readers of the same call (the fused e2 finish pass) read `base`,
// and one lane of the call's last kernel, which reads neither word, adds the call's advance to `counter`.
struct RndState {
  u32 seed[8];
  u64 counter;
  u64 base;
};
// call_seed(S, c): words 0..7 of the ChaCha8 block keyed by S with block counter c and stream id (DOM_CALL << 32) | 0
PVW_HD ChaChaKey call_seed(const u32 seed[8], u64 c) {
  ChaChaKey k;
#pragma unroll
  for (int i = 0; i < 8; ++i) k.w[i] = seed[i];
  ChaChaRng g;
  g.init(k, DOM_CALL, 0);
  g.counter = c;
  g.refill();
#pragma unroll
  for (int i = 0; i < 8; ++i) k.w[i] = g.buf[i];
  return k;
}
// one lane of the whole grid adds `adv` to the state's counter (the kernel must not read the counter itself)
__device__ __forceinline__ void rnd_advance(u64* ctr, u64 adv) {
  if (ctr && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *ctr += adv;
}

// per-context device tables (all device pointers)
struct DevTables {
  const Mod* mods;   // [L]
  const u64* tw;     // [L][l]  psi^bitrev(i)
  const u64* itw;    // [L][l]  psi^-bitrev(i)
  const u64* linv;   // [L]     l^-1 mod q
  const u64* ghat;   // [L][l]  NTT(gadget)              (parameters.rs:288-308)
  const u64* gpow;   // [L][l]  gadget residues D^j mod q (power basis)
  // Shoup companions floor(x * 2^64 / q) of the five tables above
  const u64* twp;
  const u64* itwp;
  const u64* linvp;
  const u64* ghatp;
  const u64* gpowp;
  u32 min_q_bits;    // bit length of the smallest modulus (kernels with a fast path for wide moduli test it)
  u32 max_q_bits;    // ... of the widest one (packed stream width; byte count of the digit GEMM)
};

enum { SAMPLE_CBD = 0, SAMPLE_UNIFORM = 1 };
struct SampleJob {
  u32 kind;       // SAMPLE_CBD | SAMPLE_UNIFORM
  u32 domain;     // ChaCha stream domain
  u32 index0;     // first polynomial index (stream id low word)
  u32 count;      // polynomials
  u32 out_poly0;  // first output polynomial slot
  u32 cbd_half;   // variance == 0.5 special case
  u32 cbd_v;      // (usize)variance otherwise
  u64 bound;      // uniform bound
};

// one section of the streamed tiled matrix: out[row] = sum_j M[row][j]*rhat[j] + addend[row]
// (addend may alias out; NULL = none).  A default-constructed section has no rows.
struct MacSection {
  const u64* M = nullptr;
  const u64* addend = nullptr;
  u64* out = nullptr;
  u32 nrows = 0;
  u32 row_blocks = 0;   // the launcher's: row blocks of 128 / l rows
  MacSection() = default;
  MacSection(const u64* M_, const u64* addend_, u64* out_, u32 nrows_) : M(M_), addend(addend_), out(out_), nrows(nrows_) {}
  // l <= 16: the addend of row i in COMPACT form instead of `addend` -- the l small coefficients of its error polynomial
  // (e_small[i][l], as sampled or as the caller supplied them) and, for c2 rows, the scalar m_i (scalars[i]; NULL: none).
  // The kernel transforms them itself (NTT(e_i) + m_i g-hat for its limb: encryption.rs:161-167, :195-196) -- 8 l + 8
  // bytes per row cross memory instead of 8 L l written by the prologue and read back here.
  const i64* e_small = nullptr;
  const u64* scalars = nullptr;
  // not NULL (section a): one lane adds rnd_adv to this RndState counter (the call's last kernel; see RndState)
  u64* rnd_ctr = nullptr;
  u64 rnd_adv = 0;
};
// group != 0: polynomial p goes to out + (p / group) * stride_group + (p % group) * stride_poly
hipError_t launch_prep(const i64* coeffs, const u64* scalars, u64* out, size_t stride_poly,
                       size_t stride_limb, u32 count, bool do_ntt, const DevTables& t, u32 L,
                       u32 ell, hipStream_t s, u32 group = 0, size_t stride_group = 0);
// dst[c][j] = src[j][c] for a k x k matrix of polynomials of `words` u64 each
hipError_t launch_transpose_polys(const u64* src, u64* dst, u32 k, u32 words, hipStream_t s);
hipError_t launch_ntt(u64* polys, size_t count, bool inverse, const DevTables& t, u32 L, u32 ell,
                      hipStream_t s);
hipError_t launch_tile(const u64* src, u64* M, u32 rows, u32 row0_tiled, u32 k, u32 L, u32 ell,
                       bool ntt_first, const DevTables& t, hipStream_t s);
hipError_t launch_untile(const u64* M, u64* dst, u32 rows, u32 row0_tiled, u32 k, u32 L, u32 ell,
                         bool intt_after, const DevTables& t, hipStream_t s);
hipError_t launch_fill_uniform_tiled(u64* M, const ChaChaKey& key, u32 domain, u32 rows,
                                     u32 row0_tiled, u32 grow0, u32 k, u32 L, u32 ell,
                                     const DevTables& t, hipStream_t s);
// one family of small polynomials of the encrypt prologue: sampled (explicit_coeffs == NULL) or
// supplied, reduced + transformed into out[p*stride_poly + limb*stride_limb + slot],
// optionally with scalars[p] * g-hat added (encode_scalar, parameters.rs:346-367)
struct PrologueJob {
  SampleJob sj;
  const i64* explicit_coeffs;
  const u64* scalars;
  u64* out;
  size_t stride_poly, stride_limb;
  u32 key_idx;   // which key of the batch seeds this family (replica r uses key_idx + r * rep_key)
  // replication (PrologueBatch::reps > 1): what replica r adds to the fields above
  u32 rep_key;        // 0: every replica shares the key, 1: one key per replica
  u32 rep_index0;     // stream index offset per replica
  size_t rep_out, rep_scalars, rep_coeffs;   // element offsets per replica
  // not NULL: the family is only SAMPLED -- polynomial p's l coefficients go to raw_out[p * l ..] as they are (no reduction, no
  // transform; `out`, `scalars` and the strides are not used).  Single replica only.
  i64* raw_out;
};
#define PVW_MAX_PROLOGUE_JOBS 8
#define PVW_MAX_PROLOGUE_KEYS 64
// The polynomial families of ONE encrypt (r, e1, e2) or ONE key generation (s, e), replicated `reps` times
// with regular strides (up to 64 dealers / parties per launch); the whole batch travels in the
// kernel-argument segment (< 4 KiB)
struct PrologueBatch {   // sizeof must stay below the 4 KiB kernel-argument limit
  PrologueJob job[PVW_MAX_PROLOGUE_JOBS];
  ChaChaKey key[PVW_MAX_PROLOGUE_KEYS];
  u32 njobs;
  u32 reps;    // 0 is read as 1
  u32 total;   // filled in by the launcher (polynomials per replica)
  u32 key_window, key_rep;   // filled in by the launcher: replica r reads keys [r * key_rep, r * key_rep + key_window)
  // not NULL: key i of replica r is call_seed(S, counter + rnd_off + r * key_rep + i), derived by each workgroup from the
  // device state when it runs (key[] is not read); block (0, 0) also copies counter to RndState::base
  RndState* rnd;
  u64 rnd_off;
};
hipError_t launch_prologue(const PrologueBatch& batch, const DevTables& t, u32 L, u32 ell, hipStream_t s);
// st->counter = counter, ordered on s
hipError_t launch_rnd_set_counter(RndState* st, u64 counter, hipStream_t s);

// c1 (section a: A-hat rows) and c2 (section b: B-hat rows) in a single launch
hipError_t launch_mac_rows(const MacSection& a, const MacSection& b, const u64* rhat, const DevTables& t, u32 k, u32 L, u32 ell,
                           hipStream_t s);
// the same over the PACKED copy of the sections (`width` bits per residue; MacSection::M = the packed copy).
// packed_width: the stream width for a modulus chain whose widest modulus has max_q_bits bits -- 40 / 48 / 56 (k a
// multiple of 64) or 61 (k a multiple of 256), l <= 16 -- or 0 when the geometry does not qualify.  launch_pack
// builds the copy from the tiled matrix: packed_words(rows, ..., width) u64 per section.
u32 packed_width(u32 max_q_bits, u32 k, u32 ell);
hipError_t launch_mac_rows_packed(const MacSection& a, const MacSection& b, const u64* rhat, const DevTables& t, u32 k, u32 L,
                                  u32 ell, u32 width, hipStream_t s);
// *wide_flag (device word, zeroed by the caller) is set when a matrix word does not fit `width` bits: the copy is then unusable
hipError_t launch_pack(const u64* M, u64* P, u32 rows, u32 k, u32 L, u32 ell, u32 width, u32* wide_flag, hipStream_t s);
inline size_t packed_words(u32 rows, u32 k, u32 L, u32 ell, u32 width) {
  const u32 R = 128 / ell;
  return (size_t)((rows + R - 1) / R) * L * (k / 64 * width) * 128;
}
// NV (<= 4) vectors sharing one pass over the tiled matrix (mac_rows_multi)
struct MultiVec {
  const u64* vhat;      // [nv][L][k][l]
  size_t vstride;       // words between consecutive vectors
  size_t out_stride_a;  // words between consecutive vectors' outputs / addends, section a
  size_t out_stride_b;  // ... section b
  u32 nv;
};
hipError_t launch_mac_rows_multi(const MacSection& a, const MacSection& b, const MultiVec& mv,
                                 const DevTables& t, u32 k, u32 L, u32 ell, hipStream_t s);
hipError_t launch_sample(i64* out, const ChaChaKey& key, u32 ell, const SampleJob& j0,
                         const SampleJob& j1, const SampleJob& j2, hipStream_t s);
hipError_t launch_gaussian(i64* out, const ChaChaKey& key, u32 index0, u32 count, u64 bound,
                           hipStream_t s);
// nsplit > 1 (from decrypt_split; `partial` then holds nsplit x dealers polynomials): the k terms are cut into nsplit
// ranges whose sums go to `partial`; launch_decrypt_finish adds them up, subtracts c2 and transforms back.
// nsplit <= 1: noisy = <s-hat, c1> - c2 in the NTT domain, as before (follow with launch_ntt(inverse)).
// alone = false: another kernel (the decode of the previous chunk) is meant to share the CUs with this launch: the
// register-lean instance is used (pvw_decrypt.hip).
u32 decrypt_split(u32 k, u32 L, u32 ell, size_t dealers);
hipError_t launch_decrypt_mac(const u64* c1s, const u64* shat, const u64* c2col, u64* noisy,
                              const DevTables& t, u32 k, u32 L, u32 ell, size_t dealers,
                              hipStream_t s, u64* partial = nullptr, u32 nsplit = 1, bool alone = true);
hipError_t launch_decrypt_finish(const u64* partial, u32 nsplit, const u64* c2col, u64* noisy, const DevTables& t, u32 L, u32 ell,
                                 size_t dealers, hipStream_t s);

// ---- sum of dealers' ciphertexts (pvw_sum.hip): out = sum over the valid dealers d of in + d * stride, word by word mod q ----
// One region of the sum: `items` 16-byte items (two words of one limb) per dealer, dealer d's at in + d * stride words; a
// whole number of polynomials starting on a polynomial boundary (item i is in limb (2 i mod L l) / l).  c1 is one region
// (stride k L l), the c2 rows [row_lo, row_hi) of whole ciphertexts (in = c2s + row_lo L l, stride n L l) or one party's
// column (stride L l) the other; both travel in ONE launch.
struct SumRegion {
  const u64* in = nullptr;
  u64* out = nullptr;
  size_t stride = 0;    // words between consecutive dealers (even)
  size_t items = 0;
};
#define PVW_SUM_MAX_SLICES 64
// slices of dealers (gridDim.y) for `items` items in all: 1 = unsplit.  With nslices > 1 `partial` holds nslices x items
// 16-byte slice sums and ct_sum_finish adds them up.  Bounded: nslices * items <= ct_sum_partial_items_max().
u32 ct_sum_slices(size_t items, size_t dealers);
inline size_t ct_sum_partial_items_max() { return (size_t)(1024 + 512) * 256; }   // (1024 / wgs + 1) * wgs workgroups, wgs < 512
// valid: NULL = every dealer, else valid[d] != 0 (device bytes, read when the kernel runs).  accumulate: out += the sum
// (out holds an earlier piece's result).  count: NULL, or receives the number of dealers summed.  dealers < 2^32.
hipError_t launch_ct_sum(const SumRegion& a, const SumRegion& b, const unsigned char* valid, size_t dealers, const DevTables& t, u32 L,
                         u32 ell, u64* partial, u32 nslices, bool accumulate, u32* count, hipStream_t s);
// The weighted form: out = sum over the PARTICIPATING dealers (valid and weights[d] != 0) of weights[d] * in_d,
// weights[d] any int64 read as the integer it is (device words, read when the kernel runs).  Regions, slices, partial,
// accumulate as launch_ct_sum; count receives the number of participating dealers.
hipError_t launch_ct_lincomb(const SumRegion& a, const SumRegion& b, const unsigned char* valid, const i64* weights, size_t dealers,
                             const DevTables& t, u32 L, u32 ell, u64* partial, u32 nslices, bool accumulate, u32* count,
                             hipStream_t s);
// Many combinations of the same dealers: row r of weights [nrows][wstride] (2 <= nrows < 2^31) gives what
// launch_ct_lincomb gives with weights + r * wstride, written r * out_stride_a / _b words behind a.out / b.out, and counts[r].
// One pass over the dealers per tile of ct_lincomb_many_tile(items, nslices) rows (2 or 4, by the shape), the last rows in
// narrower passes; the split form needs nslices * tile * items <= ct_sum_partial_items_max().
u32 ct_lincomb_many_tile(size_t items, u32 nslices);
hipError_t launch_ct_lincomb_many(const SumRegion& a, const SumRegion& b, size_t out_stride_a, size_t out_stride_b,
                                  const unsigned char* valid, const i64* weights, size_t wstride, size_t nrows, size_t dealers,
                                  const DevTables& t, u32 L, u32 ell, u64* partial, u32 nslices, bool accumulate, u32* counts,
                                  hipStream_t s);

// ---- Shamir shares (pvw_shamir.hip): shares[d * row_stride + i] = f_d(i + 1) mod m.q for the dealers of the batch
// and the parties i of [party_lo, party_hi); f_d = secrets[d] + sum_{j=1..degree} a_{d,j} x^j.  a_{d,j} = coeffs[d * degree + j - 1]
// (any word, read mod m.q), or with coeffs == NULL the first accepted draw of the ChaCha8 stream (key of dealer d,
// (DOM_SHAMIR << 32) | j).  Dealer d's key is key[d], or with rnd != NULL call_seed(S, counter + rnd_off + d), derived when the
// kernel runs (the kernel does not write the state).  nd <= PVW_MAX_PROLOGUE_KEYS; m.q prime, party_hi < m.q < 2^62.
// Packed, pack = K != 0: K secrets per dealer at the points 0, -1, ..., -(K-1),
//   f_d(x) = sum_{j<K} secrets[d * K + j] L_j(x) + Z(x) (a_{d,1} + a_{d,2} x + ... + a_{d,t} x^(t-1)),  Z(x) = x (x+1) ... (x+K-1),
// L_j the Lagrange basis polynomial of -j among those points; K = 1 is the polynomial above.  The weights are public and made
// on the device from (p, K, party range) alone:
// words: Lw [K][cols] | zt [cols] | w [K] | 1/j! [K], cols = party_hi - party_lo; Lw[j][i] = L_j(party_lo + i + 1),
// zt[i] = prod_{m=1..K-1}(party_lo + i + 1 + m) = Z(x) / x.  m.q prime, party_hi + K - 1 < m.q < 2^62.
enum { DOM_SHAMIR = 9 };
inline size_t shamir_packed_words(size_t pack, size_t cols) { return (pack + 1) * cols + 2 * pack; }
struct ShamirBatch {
  const u64* secrets;   // [nd], packed [nd][pack]: device words, read mod m.q
  const u64* coeffs;    // [nd][degree] device words, or NULL: drawn
  u64* shares;
  size_t row_stride;    // words between consecutive dealers' rows (columns are GLOBAL party indices)
  u32 nd, degree, party_lo, party_hi;
  Mod m;
  ChaChaKey key[PVW_MAX_PROLOGUE_KEYS];
  const RndState* rnd;
  u64 rnd_off;
  u32 pack;             // 0: the unpacked kernel, which reads neither Lw nor zt; >= 1: the packed one, whatever pack
  const u64* Lw;        // [pack][party_hi - party_lo]
  const u64* zt;        // [party_hi - party_lo]
};
hipError_t launch_shamir_packed_weights(u64* ws, u32 pack, u32 party_lo, u32 party_hi, const Mod& m, hipStream_t s);
hipError_t launch_shamir_eval(const ShamirBatch& b, hipStream_t s);

// ---- Shamir shares over a prime below 2^256 (pvw_shamir.hip): elements of four words, pvw_wide.h.
// Dealers [d_lo, d_lo + nd) of the arrays; dealer d's key is key[d - d_lo], or with rnd != NULL
// call_seed(S, counter + rnd_off + (d - d_lo) * key_stride).
// num_limbs == 0: the shares themselves, out[(d * row_stride + party) * 4 + word].
// num_limbs >= 1: limb w of dealer d is row v = d * num_limbs + w; the rows of [v0, v0 + nv) are stored, row v at
// out[(v - v0) * row_stride + party], and nothing else is written.
struct ShamirWideBatch {
  const u64* secrets;   // [*][4] device words, read mod p
  const u64* coeffs;    // [*][degree][4] device words, or NULL: drawn
  u64* out;
  size_t row_stride;
  u32 d_lo, nd, degree, party_lo, party_hi;
  u32 limb_bits, num_limbs, v0, nv;
  WideMod m;
  ChaChaKey key[PVW_MAX_PROLOGUE_KEYS];
  const RndState* rnd;
  u64 rnd_off;
  u32 key_stride;
};
hipError_t launch_shamir_eval_wide(const ShamirWideBatch& b, hipStream_t s);
// packed dealing: the batch above with secrets [*][pack][4], and the weights.  A type of its own, so the unpacked
// kernel keeps the arguments it had.
struct ShamirWidePackedBatch {
  ShamirWideBatch b;
  u32 pack;             // >= 1
  const u64* Lw;        // [pack][party_hi - party_lo][4], times 2^256 mod p
  const u64* zt;        // [party_hi - party_lo][4], likewise
  WideMont mm;          // the constants of the general product
};
hipError_t launch_shamir_eval_packed_wide(const ShamirWidePackedBatch& b, hipStream_t s);
// The weights of packed wide shares, public: Lw [pack][cols][4] | zt [cols][4] | w R^3 [pack][4] | 1/j! [pack][4], cols = party_hi - party_lo.
// party_hi + pack - 1 < 2^32 and party_hi + pack <= p.
inline size_t shamir_packed_wide_words(size_t pack, size_t cols) { return 4 * ((pack + 1) * cols + 2 * pack); }
hipError_t launch_shamir_packed_wide_weights(u64* ws, u32 pack, u32 party_lo, u32 party_hi, const WideMod& m, const WideMont& mm, hipStream_t s);
// out[i] = (acc[i] x[i] + add[i]) mod p by the kernel's own step; acc, add < p, x < 2^32 (pvw_selftest_shamir_wide_step)
hipError_t launch_shamir_wide_step(const WideMod& m, const u64* acc, const u64* x, const u64* add, size_t count, u64* out, hipStream_t s);

// ---- Checked reconstruction over a prime below 2^256 (pvw_shamir.hip): the layout of 8.10 below with elements of
// four words.  Workspace words: x [count][4] | aux [count + 1][4] | W [t+1][T][4], ALL in Montgomery form (v 2^256 mod p,
// pvw_wide.h), so that a plain share times a stored weight is one REDC away from the plain product.
inline size_t shamir_interp_wide_words(size_t count, u32 t) { return 4 * (2 * count + 1 + ((size_t)t + 1) * (count - t)); }
struct ShamirInterpWide {
  const u64* shares;     // element (s, c): four words at shares + 4 (s * secret_stride + c * point_stride), any words, read mod p
  size_t secret_stride, point_stride;
  const u64* W;          // [t+1][T][4]
  u64* out;              // [ns][4]
  u32* bad;              // [ns] or NULL; zeroed by the caller (launch_shamir_zero_counts), the kernel adds
  u32* col_bad;          // [count] or NULL; likewise
  u32 ns, degree, T;
  WideMont m;
};
// x[i] = (indices[i] + 1) 2^256 mod p, four words each (the point of index 2^64 - 1 is 2^64)
hipError_t launch_shamir_points_wide(const u64* indices, size_t count, u64* x, const WideMont& m, hipStream_t s);
hipError_t launch_shamir_weights_wide(u64* ws, size_t count, u32 degree, const WideMont& m, hipStream_t s);
hipError_t launch_shamir_interp_wide(const ShamirInterpWide& b, hipStream_t s);
// out[i] = sum_w limbs[w * limb_stride + i * elem_stride] 2^(w limb_bits) mod p, [count][4]; any words
hipError_t launch_shamir_wide_fold(const WideMod& m, const u64* limbs, size_t count, size_t limb_stride, size_t elem_stride, u32 limb_bits,
                                   u32 num_limbs, u64* out, hipStream_t s);
// out[i] = a[i] b[i] mod p by the kernels' own product; a, b < p (pvw_selftest_shamir_wide_mul)
hipError_t launch_shamir_wide_mul(const WideMont& m, const u64* a, const u64* b, size_t count, u64* out, hipStream_t s);

// ---- Checked reconstruction (pvw_shamir.hip).  Columns 0..t of the share matrix are the basis, columns
// t+1..count-1 the extras; T = count - t targets: target 0 is x = 0, target m >= 1 the point of column t + m.
// Workspace words: x [count] | aux [count + 1] | W [t+1][T].  aux[j] = (prod_{i != j}(x_j - x_i))^-1 for j <= t and
// aux[t + 1 + m] = prod_i (x_m - x_i) over the basis; W[j][m] = L_j(x_m), the basis polynomial of column j at target m.
inline size_t shamir_interp_words(size_t count, u32 t) { return 2 * count + 1 + ((size_t)t + 1) * (count - t); }
#define PVW_SHAMIR_POINTS 256                            // indices per launch of the point upload (kernel arguments)
struct ShamirPoints {
  u64 index[PVW_SHAMIR_POINTS];   // party indices; x = index + 1
  u64* x;                         // where the first of them goes
  u32 n;
};
struct ShamirInterp {
  const u64* shares;     // element (s, c) at shares[s * secret_stride + c * point_stride], any word, read mod m.q
  size_t secret_stride, point_stride;
  const u64* W;          // [t+1][T]
  u64* out;              // [ns]
  u32* bad;              // [ns] or NULL; zeroed by the caller (launch_shamir_zero_counts), the kernel adds
  u32* col_bad;          // [count] or NULL; likewise
  u32 ns, degree, T;
  Mod m;
};
hipError_t launch_shamir_zero_counts(u32* p, size_t n, hipStream_t s);   // p[0 .. n) = 0, as a kernel launch on s
hipError_t launch_shamir_points(const u64* indices, size_t count, u64* x, hipStream_t s);
hipError_t launch_shamir_weights(u64* ws, size_t count, u32 degree, const Mod& m, hipStream_t s);
hipError_t launch_shamir_interp(const ShamirInterp& b, hipStream_t s);

// ---- Corrected reconstruction (pvw_shamir.hip).  r = count - t - 1 redundant columns, E = r / 2 correctable.
// Public workspace words, from the indices alone: x [count] | aux [count + 1] (u_c, then prod_i(-x_i)) | lambda [count] |
// V [count][r] (u_c x_c^j) | X [nk][count] (x_c^k).  nk is the locator capacity of the call: E + 1, or r + 1 with erasures
// (DESIGN 8.16).
inline size_t shamir_correct_public_words(size_t count, u32 t, size_t nk) { return 3 * count + 1 + count * (count - t - 1) + nk * count; }
#define PVW_SHAMIR_NO_LOCATOR 0xFFFFFFFFu                // L of a row whose locator would need more than E coefficients
#define PVW_SHAMIR_MAX_LOCATOR 4096                      // E + 1 at most: two polynomials of one wave in 64 KiB of LDS
struct ShamirMatmul {
  const u64* A;          // element (s, j) at A[s * secret_stride + j * term_stride], any word, read mod m.q
  size_t secret_stride, term_stride;
  const u64* W;          // [terms][T]
  u64* out;              // [ns][T]
  u32 ns, terms, T;
  Mod m;
};
struct ShamirFinish {
  const u64* shares;     // as ShamirInterp
  size_t secret_stride, point_stride;
  const u64* M;          // [ns][count]: the locator of row s at every point
  const u64* Lam;        // [ns][E+1]: the reversed locators
  const u32* L;          // [ns]: their degrees, or PVW_SHAMIR_NO_LOCATOR
  const u64* lam;        // [count]: Lagrange weights at 0 over all columns
  u64* out;              // [ns]
  u32* nerr;             // [ns] or NULL
  u32* col_err;          // [count] or NULL; zeroed by the caller, the kernel adds
  u64* mask;             // [ns][ceil(count / 64)] or NULL; every word is stored
  u32 count, E;
  Mod m;
};
hipError_t launch_shamir_correct_weights(u64* ws, size_t count, u32 degree, u32 nk, const Mod& m, hipStream_t s);
hipError_t launch_shamir_matmul(const ShamirMatmul& b, hipStream_t s);
hipError_t launch_shamir_bm(const u64* synd, u64* lam, u32* L, u32 ns, u32 r, const Mod& m, hipStream_t s);
hipError_t launch_shamir_correct_finish(const ShamirFinish& f, u32 ns, hipStream_t s);

// ---- Evaluation of the corrected polynomials (pvw_shamir.hip): values[s][j] = F_s(x*_j) for a group of Tg targets,
// behind the decode above.  With G_s = F_s Lambda_s (degree <= count - 1, G_s(x_c) = y_c M[s][c]):
//   raw[s][j] = sum_i YM[s][i] C[i][j],  YM = y o M,  C[i][j] = u_i / (x*_j - x_i) (0 where the points coincide)
//   G_s(x*_j) = scale_j raw[s][j] off the points, G_s'(x_c) likewise at a point x*_j = x_c; scale_j = prod_{x_i != x*_j}(x*_j - x_i)
// Public workspace words of a group, from the indices and targets alone:
//   xt [Tg] | scale [Tg] | C [count][Tg] | Xt [nk][Tg] (x*^k) | Xd [nk][Tg] (k x*^(k-1)) | coin [Tg] (u32)
#define PVW_SHAMIR_NO_COLUMN 0xFFFFFFFFu                 // coin[j] of a target that is no column's point
inline size_t shamir_evaluate_public_words(size_t count, size_t Tg, size_t nk) { return 2 * Tg + count * Tg + 2 * nk * Tg + (Tg + 1) / 2; }
struct ShamirEvalFinish {
  const u64* shares;     // as ShamirInterp
  size_t secret_stride, point_stride;
  const u64* M;          // [ns][count]
  const u32* nerr;       // [ns]: PVW_SHAMIR_NO_LOCATOR for an undecodable row
  const u64* raw;        // [ns][Tg]
  const u64* LamT;       // [ns][Tg]: Lambda_s(x*_j)
  const u64* LamD;       // [ns][Tg]: Lambda_s'(x*_j)
  const u64* scale;      // [Tg]
  const u32* coin;       // [Tg]: the column whose point target j is, or PVW_SHAMIR_NO_COLUMN
  u64* values;           // element (s, j) at values[s * value_stride + j]
  size_t value_stride;
  u32 ns, count, Tg;
  Mod m;
};
// ws: the group's public words; x, aux: the call's points and u_c (launch_shamir_correct_weights)
hipError_t launch_shamir_evaluate_weights(const u64* x, const u64* aux, u64* ws, size_t count, u32 nk, size_t Tg, const Mod& m,
                                          hipStream_t s);
// YM[s][c] = y[s][c] M[s][c]
hipError_t launch_shamir_ym(const u64* shares, size_t secret_stride, size_t point_stride, const u64* M, u64* YM, u32 ns, u32 count,
                            const Mod& m, hipStream_t s);
hipError_t launch_shamir_evaluate_finish(const ShamirEvalFinish& f, hipStream_t s);

// ---- Reconstruction with erasures (pvw_shamir.hip): erased[s][W], W = ceil(count / 64), bit c % 64 of word c / 64
// set where share (s, c) is known to be bad.  The frame of the corrected decode with a locator capacity of nk = r + 1 instead of
// E + 1: the errata locator Psi_s = Gamma_s Lambda_s of a row has up to r + 1 coefficients.
struct ShamirMaskedMatmul : ShamirMatmul {
  const u64* erased;     // [ns][ewords]: element (s, j) of A is read as 0 where bit j of row s is set
  u32 ewords;
};
hipError_t launch_shamir_matmul_masked(const ShamirMaskedMatmul& b, hipStream_t s);
// synd [ns][r] is overwritten (the Forney syndromes take the place of a row's upper part); psi [ns][r + 1] reversed like Lambda,
// L [ns] = eps_s + deg Lambda_s or PVW_SHAMIR_NO_LOCATOR; x [count] the points
hipError_t launch_shamir_bm_erasures(u64* synd, const u64* erased, const u64* x, u64* psi, u32* L, u32 ns, u32 count, u32 r, const Mod& m,
                                     hipStream_t s);
// f as for launch_shamir_correct_finish with Lam = psi, E = r (rows r + 1 words apart) and L from launch_shamir_bm_erasures
hipError_t launch_shamir_erasures_finish(const ShamirFinish& f, const u64* erased, u32 ns, hipStream_t s);
// mask[s][w] for all w < ceil(count / 64): bit (s, c) set iff status[..] & status_bits or noise[..] > noise_bound, element (s, c) of
// either array (one may be NULL) at s * secret_stride + c * point_stride; padding bits 0
hipError_t launch_shamir_erasure_mask(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound, u32 count, u32 ns,
                                      size_t secret_stride, size_t point_stride, u64* mask, hipStream_t s);

// ---- Corrected reconstruction over a prime below 2^256 (pvw_shamir.hip): the decode of 8.11 with elements of four
// words.  Public workspace words, all times R = 2^256 (pvw_wide.h): x [count][4] | aux [count + 1][4] | lambda [count][4] |
// V [count][r][4] | X [nk][count][4], nk = E + 1 (r + 1 with erasures, 8.21).  The syndromes are plain; the locators and M are
// times R.
inline size_t shamir_correct_wide_public_words(size_t count, u32 t, size_t nk) { return 4 * shamir_correct_public_words(count, t, nk); }
#define PVW_SHAMIR_WIDE_MAX_LOCATOR 2048                 // E + 1 at most: two polynomials of one wave in 128 KiB of LDS
struct ShamirMatmulWide {
  const u64* A;          // element (s, j): four words at A + 4 (s * secret_stride + j * term_stride), any words, read mod p
  size_t secret_stride, term_stride;
  const u64* W;          // [terms][T][4], times R
  u64* out;              // [ns][T][4]
  u32 ns, terms, T;
  WideMont m;
};
struct ShamirFinishWide {
  const u64* shares;     // as ShamirInterpWide
  size_t secret_stride, point_stride;
  const u64* M;          // [ns][count][4]: the locator of row s at every point
  const u64* Lam;        // [ns][E+1][4]: the reversed locators
  const u32* L;          // [ns]: their degrees, or PVW_SHAMIR_NO_LOCATOR
  const u64* lam;        // [count][4]: Lagrange weights at 0 over all columns
  u64* out;              // [ns][4]
  u32* nerr;             // [ns] or NULL
  u32* col_err;          // [count] or NULL; zeroed by the caller, the kernel adds
  u64* mask;             // [ns][ceil(count / 64)] or NULL; every word is stored
  u32 count, E;
  WideMont m;
};
hipError_t launch_shamir_correct_weights_wide(u64* ws, size_t count, u32 degree, u32 nk, const WideMont& m, hipStream_t s);
hipError_t launch_shamir_matmul_wide(const ShamirMatmulWide& b, hipStream_t s);
hipError_t launch_shamir_bm_wide(const u64* synd, u64* lam, u32* L, u32 ns, u32 r, const WideMont& m, hipStream_t s);
hipError_t launch_shamir_correct_finish_wide(const ShamirFinishWide& f, u32 ns, hipStream_t s);
// the dynamic-LDS limits of the wide Berlekamp-Massey kernels; once per context after hipSetDevice, beside init_kernel_attributes
hipError_t init_shamir_attributes();

// ---- Reconstruction with erasures over a prime below 2^256 (pvw_shamir.hip): the decode of 8.16 with elements of
// four words, in the forms of 8.20 (public operands times R, shares and syndromes plain).  erased[s][W] as above; the locator
// capacity is nk = r + 1, so X has r + 1 rows and a row of psi r + 1 elements.
struct ShamirMaskedMatmulWide : ShamirMatmulWide {
  const u64* erased;     // [ns][ewords]: element (s, j) of A is not loaded and counts as 0 where bit j of row s is set
  u32 ewords;
};
hipError_t launch_shamir_matmul_masked_wide(const ShamirMaskedMatmulWide& b, hipStream_t s);
// synd [ns][r][4] is overwritten (the Forney syndromes take the place of a row's upper part); psi [ns][r + 1][4] reversed like
// Lambda and times R, L [ns] = eps_s + deg Lambda_s or PVW_SHAMIR_NO_LOCATOR; x [count][4] the points times R.
// r + 1 <= 2 PVW_SHAMIR_WIDE_MAX_LOCATOR: Gamma, C and B of one wave take at most r + 3 elements of LDS.
hipError_t launch_shamir_bm_erasures_wide(u64* synd, const u64* erased, const u64* x, u64* psi, u32* L, u32 ns, u32 count, u32 r,
                                          const WideMont& m, hipStream_t s);
// f as for launch_shamir_correct_finish_wide with Lam = psi, E = r (rows r + 1 elements apart) and L from the kernel above
hipError_t launch_shamir_erasures_finish_wide(const ShamirFinishWide& f, const u64* erased, u32 ns, hipStream_t s);
// launch_shamir_erasure_mask with an OR over the num_limbs elements limb_stride apart that make one share
hipError_t launch_shamir_wide_erasure_mask(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound, u32 count, u32 ns,
                                           size_t secret_stride, size_t point_stride, u32 num_limbs, size_t limb_stride, u64* mask,
                                           hipStream_t s);

// ---- Evaluation of the corrected polynomials over a prime below 2^256 (pvw_shamir.hip): the evaluation of 8.13
// with elements of four words behind the decode of 8.20 or 8.21.  Public workspace words of a group of Tg targets, all times R:
//   xt [Tg][4] | scale [Tg][4] | C [count][Tg][4] | Xt [nk][Tg][4] | Xd [nk][Tg][4] | coin [Tg] (u32)
// YM and raw are plain, the locator's values at the targets are times R like M.
inline size_t shamir_evaluate_wide_public_words(size_t count, size_t Tg, size_t nk) {
  return 4 * (2 * Tg + count * Tg + 2 * nk * Tg) + (Tg + 1) / 2;
}
struct ShamirEvalFinishWide {
  const u64* shares;     // as ShamirInterpWide
  size_t secret_stride, point_stride;
  const u64* M;          // [ns][count][4]
  const u32* nerr;       // [ns]: PVW_SHAMIR_NO_LOCATOR for an undecodable row
  const u64* raw;        // [ns][Tg][4]
  const u64* PsiT;       // [ns][Tg][4]: Psi_s(x*_j)
  const u64* PsiD;       // [ns][Tg][4]: Psi_s'(x*_j)
  const u64* scale;      // [Tg][4]
  const u32* coin;       // [Tg]: the column whose point target j is, or PVW_SHAMIR_NO_COLUMN
  u64* values;           // element (s, j): four words at values + 4 (s * value_stride + j)
  size_t value_stride;
  u32 ns, count, Tg;
  WideMont m;
};
// ws: the group's public words, xt filled by launch_shamir_points_wide; x, aux: the call's points and u_c
hipError_t launch_shamir_evaluate_weights_wide(const u64* x, const u64* aux, u64* ws, size_t count, u32 nk, size_t Tg, const WideMont& m,
                                               hipStream_t s);
hipError_t launch_shamir_ym_wide(const u64* shares, size_t secret_stride, size_t point_stride, const u64* M, u64* YM, u32 ns, u32 count,
                                 const WideMont& m, hipStream_t s);
hipError_t launch_shamir_evaluate_finish_wide(const ShamirEvalFinishWide& f, hipStream_t s);

// ---- Handover over a prime below 2^256 (pvw_shamir.hip): the int64 weight rows of a ct_lincomb_many pass from the
// signed digits of lambda_{d,m} 2^(limb_bits w) mod p, and the fold of the decrypted digit plaintexts.  Public workspace words of
// nv valid holders and a group of Tg targets, all elements times R:
//   x [nv][4] | aux [nv + 1][4] | xt [Tg][4] | scale [Tg][4] | C [nv][Tg][4] | coin [Tg] (u32) | col [nv] (u32)
#define PVW_SHAMIR_WIDE_POINTS 64                        // target points per launch of the point upload (kernel arguments)
struct ShamirWidePoints {
  u64 pt[PVW_SHAMIR_WIDE_POINTS][4];   // points below p
  u64* x;                              // where the first of them goes, times R
  u32 n;
};
inline size_t shamir_handover_wide_words(size_t nv, size_t Tg) {
  return 4 * (2 * nv + 1 + 2 * Tg + nv * Tg) + (Tg + 1) / 2 + (nv + 1) / 2;
}
struct ShamirHandoverDigits {
  const u64* scale;      // [Tg][4]
  const u64* C;          // [nv][Tg][4]
  const u32* coin;       // [Tg]
  const u32* col;        // [nv]: the holder (of all D) that valid holder i is
  i64* weights;          // row j V + v of the group, column d NL + w: weights[(j V + v) ld + d NL + w]; zeroed by the caller
  size_t ld;             // D NL
  u32 nv, Tg, NL, V, limb_bits, digit_bits;
  WideMont m;
};
hipError_t launch_shamir_points_from_wide(const u64* points, size_t count, u64* x, const WideMont& m, hipStream_t s);
hipError_t launch_shamir_handover_columns(const u32* col, size_t count, u32* d_col, hipStream_t s);
hipError_t launch_shamir_column_weights_wide(const u64* x, u64* aux, size_t count, const WideMont& m, hipStream_t s);
hipError_t launch_shamir_cauchy_wide(const u64* x, const u64* aux, const u64* xt, u64* scale, u64* C, u32* coin, size_t count, size_t Tg,
                                     const WideMont& m, hipStream_t s);
hipError_t launch_shamir_handover_digits_wide(const ShamirHandoverDigits& a, hipStream_t s);
// digits [count][V] of values [count][4] (any words, read mod p)
hipError_t launch_shamir_signed_digits_wide(const u64* values, size_t count, u32 b, u32 V, i64* digits, const WideMont& m, hipStream_t s);
// out[i] = sum_v +-wide[i][v][ww] 2^(b v) mod p, status_out[i] = OR_v status[i][v] without PVW_DEC_NEGATIVE
hipError_t launch_shamir_wide_from_digits(const u64* wide, const u32* status, size_t count, u32 V, u32 ww, u32 b, u64* out, u32* status_out,
                                          const WideMod& m, const WideMont& mm, hipStream_t s);
// x[i] = (p - (m0 + i)) R mod p for i < count: the secret points -m of a packed wide sharing, m0 + count <= 2^32
hipError_t launch_shamir_packed_secret_points_wide(u32 m0, size_t count, u64* x, const WideMont& m, hipStream_t s);

// ---- One-word handover weights from a device-side mask (pvw_shamir.hip): weights [T][D] of the holders with
// valid[d] != 0 (NULL: all) at the targets, centred, 0 in a masked column; the mask is read when the kernels run.  Public
// workspace words of D holders and a group of Tg targets:
//   x [D] | aux [D] | xt [Tg] | scale [Tg] | C [D][Tg] | coin [Tg] (u32)
inline size_t shamir_handover_words(size_t D, size_t Tg) { return 2 * D + 2 * Tg + D * Tg + (Tg + 1) / 2; }
// aux[i] = u_i over the valid holders (0 for a masked i); *count_out (may be NULL) = the number of valid holders
hipError_t launch_shamir_masked_column_weights(const u64* x, const unsigned char* valid, u64* aux, u32* count_out, size_t count, const Mod& m,
                                               hipStream_t s);
// ws: the group's words from xt on, xt filled by launch_shamir_points; weights: the group's rows [Tg][count]
hipError_t launch_shamir_handover_weights(const u64* x, const u64* aux, const unsigned char* valid, u64* ws, size_t count, size_t Tg,
                                          i64* weights, const Mod& m, hipStream_t s);
// valid[c] = 1 iff no row r has status & status_bits or noise > noise_bound at r * row_stride + c * col_stride (one array may be
// NULL); *num_valid (may be NULL) = the number of ones
hipError_t launch_shamir_valid_mask(const u32* status, const u64* noise, u32 status_bits, u64 noise_bound, u32 count, u32 rows,
                                    size_t row_stride, size_t col_stride, unsigned char* valid, u32* num_valid, hipStream_t s);

// p[0 .. words) = 0, as a kernel launch on s
hipError_t launch_wipe_words(u64* p, size_t words, hipStream_t s);

// ---- digit GEMM on the matrix cores (see pvw_gemm.hip) ----
#ifndef PVW_GEMM_RPW
#define PVW_GEMM_RPW 1                                   // row tiles (of 32 rows) per wave
#endif
#define PVW_GEMM_ROWS_PER_WG (4 * PVW_GEMM_RPW * 32)     // 4 waves per workgroup
// XM = MFMA-tiled copy of a matrix section: [limb][slot][row tile of 32][j block of 4][64 lanes][2 u64],
// row tiles padded to whole workgroups (4 waves x PVW_GEMM_RPW row tiles).
struct GemmSection {
  const u64* XM;
  const u64* addend;   // per-vector planes, same indexing as out (may alias out; NULL = none)
  u64* out;
  u64* tmp;            // intermediate [limb][slot][16 vectors][rows padded to whole workgroups]
  u32 nrows;
  u32 rt_groups;       // filled in by the launcher
  size_t tmp_bstride;  // words of `tmp` per batch of 16 vectors (filled in by the launcher)
  // key generation: the finish pass writes vector v, GEMM row c straight into the TILED public-key matrix as
  // element (party tiled_row0 + v, column c) instead of out[] (which is then only the addend); NULL = API layout
  u64* tiled_out = nullptr;
  u32 tiled_row0 = 0;
  // tiled_swap: the GEMM ROW is the party (tiled_row0 + row) and the VECTOR the column instead
  u32 tiled_swap = 0;
  // element stride between consecutive GEMM rows in out / addend (0 = one polynomial, L * l)
  size_t row_stride = 0;
  // not NULL: the finish pass of this section adds rnd_adv to this RndState counter (one lane; see RndState)
  u64* rnd_ctr = nullptr;
  u64 rnd_adv = 0;
};
inline size_t gemm_tmp_words(u32 rows, u32 L, u32 ell) {
  return (size_t)L * ell * 16 * (((rows + PVW_GEMM_ROWS_PER_WG - 1) / PVW_GEMM_ROWS_PER_WG) * PVW_GEMM_ROWS_PER_WG);
}
inline size_t xm_words(u32 rows, u32 k, u32 L, u32 ell) {
  return (size_t)L * ell * (((rows + PVW_GEMM_ROWS_PER_WG - 1) / PVW_GEMM_ROWS_PER_WG) * (PVW_GEMM_ROWS_PER_WG / 32)) *
         ((k + 3) / 4) * 128;
}
inline size_t yd_bytes(u32 nv, u32 k, u32 L, u32 ell) { return (size_t)((nv + 3) / 4) * L * ell * ((k + 3) / 4) * 1024; }
// K tiles (32 contraction rows each) of the digit GEMM.  bytes = 8: a tile is 4 consecutive j x the 8 bytes of the matrix
// element.  bytes = 7 (every modulus below 2^56, k a multiple of 64): byte 7 of every element is zero and is left out of
// the contraction -- a tile is one byte position a < 7 of 32 consecutive j, 7 tiles per 32 j instead of 8 (gemm7_ok).
// launch_mftile with bytes = 7 reduces every element mod `mods` of its limb first (required then): a caller's word may be
// >= 2^56 while its residue is not.
inline u32 gemm_ktiles(u32 k, u32 bytes) { return bytes == 7 ? 7 * (k / 32) : (k + 3) / 4; }
inline bool gemm7_ok(u32 max_q_bits, u32 k) { return max_q_bits <= 56 && k % 64 == 0 && k >= 64; }
inline size_t sy_bytes(u32 nv, u32 L, u32 ell) { return (size_t)((nv + 3) / 4) * L * ell * 32 * sizeof(int); }
hipError_t launch_mftile(const u64* src, bool src_is_tiled, u64* XM, u32 rows, u32 k, u32 L, u32 ell, hipStream_t s, u32 bytes = 8,
                         const Mod* mods = nullptr);
// small coefficients [row][j][l] -> NTT -> MFMA-tiled raw operand in one pass (l <= 32); padding included
// Exactly one source is set: `coeffs`, or `draw` -- row r, polynomial j is then the CBD stream (key, DOM_SK, (party0 + r) * k + j)
// drawn by the thread that transforms it (cbd_half / cbd_v as SampleJob's)
struct ShatDraw {
  ChaChaKey key;
  u32 cbd_half, cbd_v;
  u32 party0;     // global index of row 0's party
};
hipError_t launch_shat_mftile(const i64* coeffs, const ShatDraw* draw, u64* XM, u32 rows, u32 k, u32 L, u32 ell, const DevTables& t,
                              hipStream_t s);
// element j of vector v at (limb, slot): vhat[v * vstride + limb * lstride + j * jstride + slot];
// lstride = jstride = 0 selects the r-hat layout [limb][j][slot] (lstride = k * l, jstride = l)
hipError_t launch_vec_digits(const u64* vhat, size_t vstride, signed char* YD, int* SY, u32 nv, u32 k, u32 L, u32 ell,
                             const DevTables& t, hipStream_t s, size_t lstride = 0, size_t jstride = 0, u32 bytes = 8);
// nv may exceed 16: batches of 16 vectors then run as extra workgroups of ONE launch (adjacent in dispatch
// order, so they share the streamed matrix tiles through L2); tmp must hold ceil(nv/16) batches.
// es_a / es_b != NULL (l <= 32): that section's finish pass adds an error term it draws or reads itself, plus the
// encoded scalar, instead of an addend from memory (gemm_finish_err_kernel).  (row, v) = (GEMM row, vector).
// The pointer is to an ARRAY: element i describes the next `span` vectors (its keys travel as kernel arguments,
// 64 at most); span == 0 covers all that are left.
struct GemmErrSource {
  u32 span;
  const i64* explicit_coeffs;       // small coefficients of (row, v) at (row * coef_row + v * coef_v) * l, or NULL: drawn
  size_t coef_row, coef_v;
  ChaChaKey key[PVW_MAX_PROLOGUE_KEYS];   // key of vector v: key[(v - first vector of this element) * key_v]
  u32 key_v;
  u32 domain, index0, index_row, index_v;   // ChaCha stream of (row, v): index0 + row * index_row + v * index_v
  u64 bound;                        // uniform in [-bound, bound]
  const u64* scalars;               // NULL, or m of (row, v) at scalars[v * scalar_v + row]: + m g-hat (encode_scalar)
  size_t scalar_v;
  // not NULL: the key of vector v is call_seed(S, base + rnd_off + (v - first vector of this element) * key_v), derived
  // once per (workgroup, vector) from the device state (key[] is not read)
  const RndState* rnd;
  u64 rnd_off;
};
hipError_t launch_gemm_digits(const GemmSection& a, const GemmSection& b, const signed char* YD, const int* SY,
                              const DevTables& t, u32 k, u32 L, u32 ell, u32 nv, size_t ostride_a, size_t ostride_b,
                              hipStream_t s, const GemmErrSource* es_a = nullptr, const GemmErrSource* es_b = nullptr, u32 bytes = 8);
// the GEMM of launch_gemm_digits alone (no finish pass): a.tmp / b.tmp receive the intermediate [limb][slot][v][row];
// rt_groups and tmp_bstride of both sections are filled in
hipError_t launch_gemm_digits_core(GemmSection& a, GemmSection& b, const signed char* YD, const int* SY, const DevTables& t, u32 k,
                                   u32 L, u32 ell, u32 nv, hipStream_t s, u32 bytes = 8);
// decrypt for many parties (pvw_decrypt_all): after launch_gemm_digits_core on section a (rows = parties, vectors = dealers'
// c1), noisy[row][v] = intermediate + offset correction - c2[v * c2_vstride + row * c2_rstride] in the NTT domain, as
// [a.nrows * nv][L][l] in (row, v) order -- the input of launch_decode(..., xf)
hipError_t launch_finish_decrypt(const GemmSection& a, const int* SY, const DevTables& t, u32 L, u32 ell, u32 nv, const u64* c2,
                                 size_t c2_vstride, size_t c2_rstride, u64* noisy, hipStream_t s);
// dst[i] = src[i] mod q of its limb, for `words` words of [.][L][l] polynomials (words even; dst may alias src)
hipError_t launch_reduce_words(const u64* src, u64* dst, size_t words, const DevTables& t, u32 L, u32 ell, hipStream_t s);
// read-only probe: every wave streams `tiles` consecutive 1-KiB tiles (16 in flight), grid as mac_rows
#if PVW_TUNING
// time stamps (100 MHz ticks, [2b] start / [2b+1] end) and HW_ID words of the workgroups of the last stamped mac_rows launch
hipError_t read_stamps(u64* out, u32* hw, u32 count);
hipError_t init_probe_attributes();
hipError_t launch_read_probe(const u64* M, size_t total_tiles, u32 tiles_per_wave, u64* sink, hipStream_t s);
hipError_t launch_read_probe2(const u64* M, size_t total_tiles, u32 tiles_per_wave, u64* sink, u32 U, bool dbuf, u32 lds_bytes,
                              hipStream_t s, u32 xmap = 0);
#endif
// per-device kernel attributes (dynamic-LDS limits); call once per context after hipSetDevice
hipError_t init_kernel_attributes();
hipError_t launch_mfma_probe(const signed char* A, const signed char* B, int* C, hipStream_t s);
// xf == nullptr: noisy holds power-basis polynomials (read only).  xf != nullptr: noisy holds them in the NTT domain; the
// decode transforms each ciphertext back as it stages it and stores the power-basis polynomial over it (the inverse
// transform of decrypt, decryption.rs:116, without a launch of its own).
// wipe / wipe_bytes (a multiple of 16): a region the decode launch clears as well (NTT(sk) of the decrypt it closes; every
// launch in front of it on `s` must be done with it); *wiped says whether this launch took that on (the fixed-width
// fallback does not).
// noise / status (either may be NULL; both NULL: the unchecked kernels): the checked decode's report per ciphertext
// (pvw_decode.h: decode_one_fixed, pvw_decode_wave.h: decode_chain_body), out[] unchanged.  A checked launch
// takes no wipe (*wiped comes back false).
// plain (NULL or no option set: none): the checked launch with the plain tail -- out[] = P mod plain->m.q and / or
// the words of |P| at plain->wide, in the same launch; the shape dispatch is the same.
hipError_t launch_decode(u64* noisy, u64* out, size_t count, const DecodeTables& t, hipStream_t s, const DevTables* xf = nullptr,
                         u64* wipe = nullptr, size_t wipe_bytes = 0, bool* wiped = nullptr, u64* noise = nullptr,
                         u32* status = nullptr, const PlainArgs* plain = nullptr);

// wire format v1 (pvw_wire.hip): `count` polynomials [L][ell] u64 <-> packed bytes (w_i = bit length of q_i bits per
// residue).  words / packed pointers 16-byte aligned; L <= 64.  Unpack: *bad += residues >= q_i (the caller zeroes it);
// words == NULL only counts.  init_wire_attributes: dynamic-LDS limit of both kernels (once per device).
hipError_t launch_wire_pack(const u64* words, size_t count, unsigned char* out, const Mod* mods, u32 L, u32 ell, hipStream_t s);
hipError_t launch_wire_unpack(const unsigned char* in, size_t count, u64* words, unsigned long long* bad, const Mod* mods, u32 L,
                              u32 ell, hipStream_t s);
hipError_t init_wire_attributes();

}  // namespace pvw

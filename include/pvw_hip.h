/* pvw_hip.h -- C ABI of the MI355X-native PVW multi-receiver encrypt/decrypt path.
 *
 * This is the drop-in boundary for the hot path of gnosisguild/pvw-rs: a Rust
 * host that keeps the `pvw::{params,crs,keys,crypto}` API binds these symbols
 * (see INTEGRATION.md for the `extern "C"` block) and every bulk polynomial
 * operation becomes one call into hand-written HIP for gfx950.  The reference
 * has no FFI of its own (no `extern`, no `unsafe`); each entry point below
 * cites the reference routine (file:line under the reference checkout) whose
 * work it replaces.
 *
 * Conventions
 *   - plain pointers and sizes; every pointer is caller-owned unless returned
 *     by a *_create; no C++/torch types.
 *   - every function returns int32_t: 0 = PVW_OK, otherwise one of the
 *     PVW_ERR_* codes, which map 1:1 onto the PvwError variants of
 *     src/errors.rs:13-70.  pvw_last_error() returns the thread-local message.
 *   - polynomial = [L][l] uint64_t, limb-major (the Array2<u64> (num_moduli,
 *     degree) of src/params/parameters.rs:433-458), residues in [0, q_i)
 *     (words >= q_i: "Residue words" below).
 *     Matrices are row-major arrays of polynomials: A is [k][k], B is [n][k].
 *   - `repr`: PVW_REPR_POWER = coefficients (fhe-math Representation::PowerBasis),
 *     PVW_REPR_NTT = this library's NTT domain (slot s of limb i holds the
 *     evaluation at psi_i^(2*bitrev(s)+1); psi_i from pvw_ctx_get_roots).  The
 *     NTT-domain layout of fhe-math is not pinned by the reference's tests, so
 *     data exchanged with an fhe-math host should cross in PVW_REPR_POWER unless
 *     pvw_ctx_set_roots() has been given fhe-math's roots.
 *   - host-buffer calls are synchronous (results are in the buffers on return)
 *     and safe to call concurrently on one context, as rayon does with
 *     `encrypt` (src/crypto/encryption.rs:277-283): device tensors are
 *     read-only after load and every call takes a stream + workspace from a pool.
 *     The promise, as tests/test_gpu_concurrent_calls.py holds it: threads that share one context may overlap any of
 *     pvw_encrypt[_rs], pvw_encrypt_multi[_rs], pvw_deal_shares[_rs], pvw_shamir_shares, pvw_deal_shares_packed[_rs],
 *     pvw_shamir_shares_packed (the concurrent calls of these: tests/test_gpu_shamir_packed.py), pvw_shamir_reconstruct_checked,
 *     pvw_shamir_reconstruct_corrected, pvw_shamir_evaluate_corrected (the concurrent calls of these two:
 *     tests/test_gpu_shamir_evaluate.py), pvw_shamir_reconstruct_erasures, pvw_shamir_evaluate_erasures (the concurrent calls of
 *     these two: tests/test_gpu_shamir_erasures.py), pvw_shamir_shares_wide, pvw_deal_shares_wide[_rs],
 *     pvw_shamir_reconstruct_wide_checked, pvw_shamir_reconstruct_wide_corrected, pvw_selftest_shamir_wide_step / _mul and, each
 *     on the calling thread's stream, pvw_shamir_shares_wide_device, pvw_deal_shares_wide[_rs]_device,
 *     pvw_shamir_wide_from_limbs_device, pvw_shamir_reconstruct_wide_checked_device / _corrected_device (the concurrent calls of
 *     this family, a context's very first calls and a count whose launch needs the raised LDS limit among them:
 *     tests/test_gpu_shamir_wide_concurrent.py), pvw_shamir_reconstruct_wide_erasures and, on the calling thread's stream,
 *     pvw_shamir_reconstruct_wide_erasures_device / pvw_shamir_wide_erasure_mask_device (the concurrent calls of these:
 *     tests/test_gpu_shamir_wide_erasures.py), pvw_shamir_evaluate_wide_corrected, pvw_shamir_evaluate_wide_erasures and, on
 *     the calling thread's stream, their _device forms (the concurrent calls of these: tests/test_gpu_shamir_wide_evaluate.py),
 *     pvw_shamir_evaluate_wide_corrected_at / _erasures_at, pvw_shamir_packed_wide_secrets and, on the calling thread's stream,
 *     their _device forms (the concurrent calls of these: tests/test_gpu_shamir_wide_points.py),
 *     pvw_decrypt_batch / _checked / _plain, pvw_decrypt_all / _checked / _plain, pvw_ct_sum, pvw_decrypt_sum_checked,
 *     pvw_decrypt_all_sum_checked, pvw_ct_lincomb, pvw_decrypt_lincomb_plain, pvw_decrypt_all_lincomb_plain (the concurrent
 *     calls of these three: tests/test_gpu_ct_lincomb.py), pvw_ct_lincomb_many, pvw_decrypt_all_lincomb_many_plain (the concurrent
 *     calls of these two, R = 1 and R > 1: tests/test_gpu_ct_lincomb_many.py), pvw_decode / _checked / _plain, pvw_wire_pack / _unpack, pvw_ntt_forward / _inverse,
 *     pvw_sample_cbd / _uniform / _gaussian, pvw_sk_load / pvw_sk_free, and *_device calls that each thread enqueues on a
 *     stream of its own -- the context's first calls included (device initialisation and the derived copies are built
 *     once, under a lock).  Every result is the serial one bit for bit, pvw_last_error stays the calling thread's, and a
 *     pooled workspace that goes from one kind of call to another carries nothing over (pvw_selftest_secret_residue).
 *     OUTSIDE the promise, because they change the resident matrices or share a caller-owned object:
 *       pvw_load_crs* / pvw_load_pk* (the _wire forms too), pvw_keygen[_seeded], pvw_pk_fill_uniform, pvw_crs_generate and
 *       pvw_ctx_set_roots next to any other call on the context (GlobalPublicKey's mutators take &mut self,
 *       public_key.rs:214-263: a change and a use never overlap);
 *       two threads drawing from one pvw_rnd_state (it is ordered by one stream at a time, see below);
 *       two threads enqueueing *_device calls on the SAME stream (the stream's workspace is protected by stream order,
 *       which two enqueueing threads do not have).
 *   - *_device calls take device pointers and a hipStream_t (as void*; NULL =
 *     the context's own stream) and enqueue asynchronously.  They do not
 *     synchronise or allocate ONCE pvw_prepare() has run for that stream since
 *     the matrices last changed.  Without pvw_prepare() the first call on a
 *     stream allocates that stream's workspace, and the first encrypt after a
 *     CRS / public-key change builds the derived copies of the matrices it
 *     streams from (a bit-packed copy for pvw_encrypt_device, an MFMA-tiled copy
 *     for pvw_encrypt_multi_device): that call allocates up to a second copy of
 *     the resident matrices and waits for the build.  A call made while its
 *     stream is being captured into a graph never builds anything: it uses the
 *     copies that are valid (pvw_prepare first) or the plain tiled matrices
 *     (multi-dealer encrypt on the matrix cores fails without pvw_prepare(PVW_PREPARE_MFMA)).
 *     A captured encrypt with PVW_RND_SEED repeats its randomness on every replay:
 *     capture the *_rs_device calls, which draw from a pvw_rnd_state, instead.
 *     The context's own stream is created non-blocking: it is NOT ordered against
 *     the legacy default stream, so a caller that prepares or consumes the buffers
 *     on the default stream (stream 0 -- also what a framework's "current stream"
 *     usually is) must either pass a stream of its own or synchronise the device
 *     between its work and the call (pvw_ctx_synchronize waits for the context's
 *     stream).
 */
#ifndef PVW_HIP_H
#define PVW_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define PVW_API __attribute__((visibility("default")))
#else
#define PVW_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pvw_ctx pvw_ctx;

/* ---- status codes <-> PvwError (src/errors.rs:13-70), in declaration order ---- */
enum {
  PVW_OK = 0,
  PVW_ERR_INVALID_PARAMETERS = 1,  /* errors.rs:15 */
  PVW_ERR_SAMPLING = 2,            /* :18 */
  PVW_ERR_ENCRYPTION = 3,          /* :21 */
  PVW_ERR_DECRYPTION = 4,          /* :24 */
  PVW_ERR_KEY_GENERATION = 5,      /* :27 */
  PVW_ERR_CRS = 6,                 /* :30 */
  PVW_ERR_SERIALIZATION = 7,       /* :33 */
  PVW_ERR_DESERIALIZATION = 8,     /* :36 */
  PVW_ERR_ENCODING = 9,            /* :39 */
  PVW_ERR_DECODING = 10,           /* :42 */
  PVW_ERR_VALIDATION = 11,         /* :45 */
  PVW_ERR_CONTEXT = 12,            /* :48 */
  PVW_ERR_POLYNOMIAL = 13,         /* :51 */
  PVW_ERR_MATRIX = 14,             /* :54 */
  PVW_ERR_DIMENSION_MISMATCH = 15, /* :57  {expected, actual} in the message */
  PVW_ERR_INDEX_OUT_OF_BOUNDS = 16,/* :60  {index, bound} in the message */
  PVW_ERR_INSUFFICIENT_DATA = 17,  /* :63 */
  PVW_ERR_INVALID_FORMAT = 18,     /* :66 */
  PVW_ERR_INTERNAL = 19            /* :69  also: HIP runtime failures, no device */
};

enum { PVW_REPR_POWER = 0, PVW_REPR_NTT = 1 };
/* Residue words.  Every uint64_t residue word w a caller passes in limb i (CRS, public keys, ciphertexts c1 / c2,
 * polynomials for the transforms, noisy residues for the decode) means w mod q_i: any 64-bit word is accepted and
 * no call checks or rejects it.  Every residue word a call returns is below q_i, with one exception: an NTT-domain
 * load (pvw_load_crs[_device] / pvw_load_pk[_device] with PVW_REPR_NTT) stores the caller's words as given, and
 * pvw_get_crs / pvw_get_pk in PVW_REPR_NTT hand those stored words back unchanged.  Signed inputs (secret-key
 * coefficients, key errors ek, explicit r / e1 / e2, scalars read as int64) mean their signed residue
 * ((c % q) + q) % q, as parameters.rs:440-443. */
enum { PVW_RND_SEED = 0, PVW_RND_EXPLICIT = 1 };

/* ChaCha8 stream-id domains of the counter-based sampler: stream = (domain<<32)|poly index */
enum {
  PVW_DOM_R = 0, PVW_DOM_E1 = 1, PVW_DOM_E2 = 2, PVW_DOM_SK = 3, PVW_DOM_EKEY = 4,
  PVW_DOM_CRS = 5, PVW_DOM_GAUSS = 6, PVW_DOM_PK = 7, PVW_DOM_CALL = 8 /* pvw_rnd_call_seed */,
  PVW_DOM_SHAMIR = 9 /* polynomial coefficients of pvw_shamir_shares* / pvw_deal_shares*: stream index = j */
};

/* PvwParametersBuilder fields (src/params/parameters.rs:44-52).  The builder's
 * defaults (variance 0.5, bounds 100/200, :166-168) are applied by the host
 * mirror; this struct always carries explicit values. */
typedef struct {
  uint32_t n;               /* set_parties   :61  (global party count)            */
  uint32_t k;               /* set_dimension :67                                  */
  uint32_t l;               /* set_l         :73  ring degree, power of two >= 8  */
  uint32_t num_moduli;      /* set_moduli    :79                                  */
  const uint64_t* moduli;
  float secret_variance;    /* set_secret_variance :85                            */
  uint64_t error_bound_1;   /* set_error_bound_1   :91  (fits u64; reference is BigInt) */
  uint64_t error_bound_2;   /* set_error_bound_2   :97                            */
  int32_t device;           /* HIP device ordinal, -1 = current device            */
  /* party shard held by this context (one process per GPU): rows [party_lo, party_hi)
   * of B / c2 and rows [c1_lo, c1_hi) of A / c1.  All zero = everything.        */
  uint32_t party_lo, party_hi;
  uint32_t c1_lo, c1_hi;
} pvw_params_t;

/* Randomness of one encrypt call.  The reference draws from thread_rng() inside
 * rayon closures (encryption.rs:138,164,180) and cannot be replayed; this ABI
 * makes the randomness an input -- it travels with the call, so a call captured into a
 * graph REPEATS it on every replay (use a pvw_rnd_state, below, for captured encrypts).  SEED: r ~ CBD(secret_variance), e1/e2 uniform
 * in [-bound, bound], each polynomial from its own ChaCha8 stream.  EXPLICIT:
 * small signed coefficients supplied by the caller. */
typedef struct {
  uint32_t mode;            /* PVW_RND_SEED | PVW_RND_EXPLICIT */
  uint8_t seed[32];
  const int64_t* r;         /* [k][l] */
  const int64_t* e1;        /* [k][l] */
  const int64_t* e2;        /* [n][l]  (global n; a sharded context reads its rows) */
} pvw_randomness_t;

/* message of the calling thread's last failure (NUL-terminated, truncated to len) */
PVW_API int32_t pvw_last_error(char* buf, size_t len);
/* 1 if a gfx950 device is usable from this process, 0 otherwise (never fails) */
PVW_API int32_t pvw_device_available(void);

/* ---- parameters: PvwParametersBuilder::build (parameters.rs:117-195) ------------
 * Validation mirrors :131-181 (n>0, k>0, l power of two >= 8, bounds > 0) plus what
 * the reference delegates to fhe-math Context::new_arc (:147): moduli distinct odd
 * primes < 2^62 with q = 1 (mod 2l). */
PVW_API int32_t pvw_ctx_create(const pvw_params_t* params, pvw_ctx** out);
PVW_API int32_t pvw_ctx_destroy(pvw_ctx* ctx);
/* psi_i (primitive 2l-th root per limb).  Default: the smallest one.  set_roots must
 * precede any load/keygen call; it lets a host align this NTT domain with another library's. */
PVW_API int32_t pvw_ctx_get_roots(const pvw_ctx* ctx, uint64_t* psi_out /*[L]*/);
PVW_API int32_t pvw_ctx_set_roots(pvw_ctx* ctx, const uint64_t* psi /*[L]*/);
/* big integers as little-endian 64-bit words; *nwords receives the count (cap = capacity) */
PVW_API int32_t pvw_ctx_delta(const pvw_ctx* ctx, uint64_t* words, size_t cap, size_t* nwords);            /* delta()  :370 */
PVW_API int32_t pvw_ctx_delta_power_l_minus_1(const pvw_ctx* ctx, uint64_t* words, size_t cap, size_t* nwords); /* :375 */
PVW_API int32_t pvw_ctx_q_total(const pvw_ctx* ctx, uint64_t* words, size_t cap, size_t* nwords);          /* q_total() :380 */
/* gadget_polynomial (parameters.rs:288-308): [1, D, ..., D^(l-1)] as one polynomial */
PVW_API int32_t pvw_ctx_gadget(const pvw_ctx* ctx, uint64_t* poly_out /*[L][l]*/, uint32_t repr);
/* verify_correctness_condition (parameters.rs:510-551) */
PVW_API int32_t pvw_ctx_verify_correctness_condition(const pvw_ctx* ctx, int32_t* ok_out);
/* the total_bound of verify_correctness_condition (parameters.rs:516-543): the three terms summed in f64 in the reference's
 * order, floored and saturated to u64.  The noise a checked decrypt reports is compared with it. */
PVW_API int32_t pvw_ctx_noise_bound(const pvw_ctx* ctx, uint64_t* out);
/* suggest_error_bounds (parameters.rs:554-603) */
PVW_API int32_t pvw_suggest_error_bounds(uint32_t n, uint32_t k, uint32_t l, const uint64_t* moduli,
                                 uint32_t num_moduli, float variance, uint32_t* bound1_out,
                                 uint32_t* bound2_out);
/* encode_scalar (parameters.rs:346-367): scalar * gadget as one polynomial */
PVW_API int32_t pvw_encode_scalar(const pvw_ctx* ctx, int64_t scalar, uint64_t* poly_out, uint32_t repr);

/* ---- CRS: PvwCrs.matrix (src/params/crs.rs:12-17) --------------------------------
 * a: host [k][k][L][l] in `repr`.  A sharded context keeps rows [c1_lo, c1_hi). */
PVW_API int32_t pvw_load_crs(pvw_ctx* ctx, const uint64_t* a, uint32_t repr);
PVW_API int32_t pvw_load_crs_device(pvw_ctx* ctx, const uint64_t* d_a, uint32_t repr, void* stream);
/* PvwCrs::new_deterministic analogue (crs.rs:45-67): uniform NTT-domain polynomials from a
 * 32-byte seed with this library's ChaCha8 streams (PVW_DOM_CRS) -- not fhe-math's bytes. */
PVW_API int32_t pvw_crs_generate(pvw_ctx* ctx, const uint8_t seed[32]);
/* PvwCrs::new_from_tag (crs.rs:74-90): the 32-byte seed the reference derives from a string tag -- the 64-bit
 * std DefaultHasher (SipHash-1-3, zero key) of tag + "CRS", little-endian, repeated four times.  Feed it to
 * pvw_crs_generate.  (PvwCrs::new, crs.rs:24-39, is pvw_crs_generate with a seed from the host's entropy source.) */
PVW_API int32_t pvw_crs_seed_from_tag(const char* tag, uint8_t seed_out[32]);
/* download: a_out host [k][k][L][l] (only rows held by this context are written) */
PVW_API int32_t pvw_get_crs(pvw_ctx* ctx, uint64_t* a_out, uint32_t repr);

/* ---- global public key: GlobalPublicKey.matrix (src/keys/public_key.rs:43-54) ----
 * add_public_key (:214-250) for parties [party_lo, party_hi): b host [count][k][L][l].
 * Bookkeeping as :245: num_keys = max(num_keys, party_hi). */
PVW_API int32_t pvw_load_pk(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const uint64_t* b,
                    uint32_t repr);
PVW_API int32_t pvw_load_pk_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi,
                           const uint64_t* d_b, uint32_t repr, void* stream);
/* synthetic uniform B-hat (benchmarks; statistically what Poly::random gives, crs.rs:32) */
PVW_API int32_t pvw_pk_fill_uniform(pvw_ctx* ctx, const uint8_t seed[32]);
PVW_API int32_t pvw_get_pk(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, uint64_t* b_out,
                   uint32_t repr);
PVW_API int32_t pvw_num_public_keys(const pvw_ctx* ctx, uint32_t* out);   /* num_public_keys :344 */
PVW_API int32_t pvw_is_full(const pvw_ctx* ctx, int32_t* out);            /* is_full :349 */

/* ---- key generation: PublicKey::generate (public_key.rs:111-147) over
 * PvwCrs::multiply_by_secret_key (crs.rs:138-171), batched as generate_all_keys
 * (public_key.rs:407-434).  b_i = s_i * A + e_i for parties [party_lo, party_hi).
 * sk: [count][k][l] CBD coefficients (SecretKey.secret_coeffs, secret_key.rs:14-18).
 * ek: [count][k][l] explicit key errors, or NULL to sample uniform[-bound1, bound1]
 * from `seed` (PVW_DOM_EKEY).  Result is stored as rows of B on the device. */
PVW_API int32_t pvw_keygen(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                   const int64_t* ek, const uint8_t seed[32]);
/* SecretKey::random (secret_key.rs:45-63) for `count` parties from a seed (PVW_DOM_SK) */
PVW_API int32_t pvw_sample_secret_keys(const pvw_ctx* ctx, const uint8_t seed[32], uint32_t party_lo,
                               uint32_t count, int64_t* sk_out /*[count][k][l]*/);
/* Key generation from a seed: GlobalPublicKey::generate_all_party_keys (public_key.rs:376-401) over Party::new /
 * SecretKey::random (public_key.rs:62-79, secret_key.rs:45-63), which draws the keys where it uses them.  b_p = s_p * A + e_p for
 * the parties of [party_lo, party_hi) this context holds, with s_p[j] the CBD polynomial of stream (sk_seed, PVW_DOM_SK,
 * p * k + j), p the GLOBAL party index -- the words pvw_sample_secret_keys(ctx, sk_seed, p, 1, .) returns -- drawn by the
 * kernel that transforms them, and e_p drawn as pvw_keygen draws it with ek == NULL (seed, PVW_DOM_EKEY).  The rows of B-hat
 * are bit-equal to pvw_sample_secret_keys + pvw_keygen(.., ek = NULL, seed); no secret key crosses the bus or exists on the
 * host.  sk_seed == seed is allowed (the domains differ).  Checks, codes and bookkeeping are pvw_keygen's; party_hi * k must be
 * below 2^32 (the stream index is 32 bits). */
PVW_API int32_t pvw_keygen_seeded(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const uint8_t sk_seed[32],
                                  const uint8_t seed[32]);
/* SecretKey::random (secret_key.rs:45-63; Party::new, public_key.rs:62-79) for `count` parties straight into caller-owned
 * device memory on the caller's stream (NULL: the context's): the words pvw_sample_secret_keys returns, with no staging, no
 * download and no synchronisation -- what the _device forms of pvw_decrypt_all* / pvw_decrypt_batch* take as d_sk.  The caller
 * clears the buffer.  (party_lo + count) * k must be below 2^32; count == 0 does nothing. */
PVW_API int32_t pvw_sample_secret_keys_device(pvw_ctx* ctx, const uint8_t seed[32], uint32_t party_lo, uint32_t count,
                                              int64_t* d_sk_out /*[count][k][l]*/, void* stream);

/* ---- encrypt (src/crypto/encryption.rs:105-214) -----------------------------------
 * Checks mirror :109 (scalar count), :117 (key fullness), :124 (correctness gate).
 * scalars: n values (global).  c1_out: [k][L][l], c2_out: [n][L][l]; a sharded context
 * writes only its rows [c1_lo,c1_hi) / [party_lo,party_hi) at their global positions.
 * `scalars[i] as i64` wraps as the reference does (:195). */
PVW_API int32_t pvw_encrypt(pvw_ctx* ctx, const uint64_t* scalars, size_t num_scalars,
                    const pvw_randomness_t* rnd, uint64_t* c1_out, uint64_t* c2_out,
                    uint32_t out_repr);
/* device-resident variant: d_scalars [n]; d_c1 [c1 rows held][L][l]; d_c2 [parties held][L][l]
 * (LOCAL row numbering); explicit randomness pointers, if used, are device pointers too. */
PVW_API int32_t pvw_encrypt_device(pvw_ctx* ctx, const uint64_t* d_scalars, size_t num_scalars,
                           const pvw_randomness_t* rnd, uint64_t* d_c1, uint64_t* d_c2,
                           uint32_t out_repr, void* stream);

/* ---- multi-dealer encrypt: encrypt_all_party_shares (src/crypto/encryption.rs:253-286) ----
 * Dealer d encrypts scalars[d][0..n) with its own randomness (seeds + 32*d, PVW_RND_SEED
 * semantics).  Dealers are processed four at a time against ONE pass over A-hat / B-hat, so
 * the public key is streamed D/4 times instead of D times.
 * scalars [D][n]; c1_out [D][k][L][l]; c2_out [D][n][L][l].  scalars_per_dealer must be n (:264-274). */
PVW_API int32_t pvw_encrypt_multi(pvw_ctx* ctx, const uint64_t* scalars, size_t num_dealers,
                                  size_t scalars_per_dealer, const uint8_t* seeds /*[D][32]*/,
                                  uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr);
/* device-resident variant: d_scalars [D][n]; d_c1 [D][c1 rows held][L][l]; d_c2 [D][parties held][L][l];
 * seeds stays a HOST pointer */
PVW_API int32_t pvw_encrypt_multi_device(pvw_ctx* ctx, const uint64_t* d_scalars, size_t num_dealers,
                                         size_t scalars_per_dealer, const uint8_t* seeds,
                                         uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream);

/* ---- encrypt from a device randomness state -----------------------------------------------------------------------
 * PVW_RND_SEED puts the seed into the kernel arguments: a call captured into a graph (hipGraph, torch.cuda.graph)
 * REPEATS its r, e1, e2 on every replay, and two replays with different scalars reveal m - m' (c1 == c1',
 * c2 - c2' = (m - m') g-hat).  The reference draws fresh randomness on every encrypt (encryption.rs:135-167).  A
 * pvw_rnd_state holds a 32-byte seed S and a 64-bit counter c on the device; encrypt calls that take one read it when
 * their kernels RUN and advance c themselves, so every replay and every queued asynchronous call draws new randomness.
 *   call_seed(S, c) = words 0..7 (little-endian bytes) of the ChaCha8 block keyed by S with block counter c and stream
 *   id (PVW_DOM_CALL << 32) | 0 (the layout of the samplers' streams); pvw_rnd_call_seed computes it on the host.
 *   pvw_encrypt_rs[_device] running while the state holds c  ==  pvw_encrypt[_device] with PVW_RND_SEED and seed
 *   call_seed(S, c); afterwards the state holds c + 1.
 *   pvw_encrypt_multi_rs[_device] with D dealers  ==  pvw_encrypt_multi[_device] with seeds[d] = call_seed(S, c + d);
 *   afterwards the state holds c + D.
 * The state is ordered by the stream of the call that uses it: it must not be used by calls on two streams at once
 * (host-buffer calls run on a pooled stream of their own and return when done: make sure earlier asynchronous work on
 * the state has completed first).  Sharded contexts (one process per GPU) that create their states with the same (S, c)
 * and make the same calls stay in step, so r stays shared across ranks.  The derived seeds never leave registers / LDS.
 * No call allocates or synchronises with the host once pvw_prepare has run for its stream (multi-dealer: under stream
 * capture without pvw_prepare(PVW_PREPARE_MFMA), the call returns PVW_ERR_INVALID_PARAMETERS and enqueues nothing).
 * Argument errors (NULL handle, dealer count, scalars_per_dealer) come before any device work. */
/* The state is an opaque handle (void*, like the buffers of pvw_host_alloc) made by pvw_rnd_state_create.
 * create allocates the state on ctx's device (not under stream capture); the handle records that device and ctx's stream
 * (used for NULL stream arguments below and by pvw_rnd_state_free) and does not read ctx again.  Free it before the context. */
PVW_API int32_t pvw_rnd_state_create(pvw_ctx* ctx, const uint8_t seed[32], uint64_t counter, void** out);
/* the counter once the work enqueued on `stream` so far is done (waits for that stream; not under capture) */
PVW_API int32_t pvw_rnd_state_counter(void* st, void* stream, uint64_t* out);
/* stream-ordered write of the counter (a one-lane kernel: may be captured) */
PVW_API int32_t pvw_rnd_state_set_counter(void* st, uint64_t counter, void* stream);
/* clears the device seed and counter (stream-ordered memset, then a wait on the recorded stream), then frees.  Work that
 * uses the state on other streams must be complete.  NULL is a no-op. */
PVW_API int32_t pvw_rnd_state_free(void* st);
/* call_seed(seed, counter) on the host (no GPU needed) */
PVW_API int32_t pvw_rnd_call_seed(const uint8_t seed[32], uint64_t counter, uint8_t out[32]);
/* as pvw_encrypt / pvw_encrypt_device, with the randomness from `st` instead of a pvw_randomness_t */
PVW_API int32_t pvw_encrypt_rs(pvw_ctx* ctx, const uint64_t* scalars, size_t num_scalars, void* st,
                               uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_encrypt_rs_device(pvw_ctx* ctx, const uint64_t* d_scalars, size_t num_scalars, void* st,
                                      uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream);
/* as pvw_encrypt_multi / pvw_encrypt_multi_device, with the dealers' seeds derived from `st` */
PVW_API int32_t pvw_encrypt_multi_rs(pvw_ctx* ctx, const uint64_t* scalars, size_t num_dealers, size_t scalars_per_dealer,
                                     void* st, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_encrypt_multi_rs_device(pvw_ctx* ctx, const uint64_t* d_scalars, size_t num_dealers,
                                            size_t scalars_per_dealer, void* st, uint64_t* d_c1, uint64_t* d_c2,
                                            uint32_t out_repr, void* stream);
/* SELF-TEST: 32-bit words of the device seed that were not zero when the calling thread's last pvw_rnd_state_free read
 * it back after clearing it (0 = cleared).  No product path calls it. */
PVW_API int32_t pvw_selftest_rnd_free_residue(uint64_t* nonzero_words);

/* ---- decrypt (src/crypto/decryption.rs:249-325) ------------------------------------
 * One secret key against D dealer ciphertexts (decrypt_party_shares :281-325):
 *   noisy_d = sum_j NTT(sk[j]) * c1s[d][j] - c2col[d]      (:257-274)
 *   out[d]  = decode_scalar_pvw_rns(noisy_d)               (:10-58)
 * sk [k][l]; c1s [D][k][L][l] and c2col [D][L][l] in `in_repr`; out_u64 [D];
 * noisy_out optional [D][L][l], power basis. */
PVW_API int32_t pvw_decrypt_batch(pvw_ctx* ctx, const int64_t* sk, const uint64_t* c1s,
                          const uint64_t* c2col, size_t num_dealers, uint32_t in_repr,
                          uint64_t* out_u64, uint64_t* noisy_out);
/* device-resident first half: d_noisy [D][L][l] power basis */
PVW_API int32_t pvw_decrypt_noisy_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s,
                                 const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                 uint64_t* d_noisy, void* stream);
/* decrypt_party_shares (decryption.rs:281-325) with device pointers end to end: d_noisy [D][L][l] is scratch /
 * optional output (power basis), d_out [D] the decoded values.  Asynchronous on `stream`; internally the decode
 * of one chunk of dealers overlaps the inner products of the next. */
PVW_API int32_t pvw_decrypt_batch_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s,
                                 const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                 uint64_t* d_noisy, uint64_t* d_out, void* stream);
/* A secret key kept on the device as the inner products read it -- NTT(sk[j]) in the ciphertext layout, what
 * SecretKey::get_polynomial computes k times per decrypt_party_value (src/keys/secret_key.rs:98-112, called at
 * src/crypto/decryption.rs:260).  decrypt_party_shares (decryption.rs:281-325) decrypts n ciphertexts under ONE key: load it
 * once, decrypt with pvw_decrypt_batch_device_sk as often as needed (no transform of the key, no wipe per call), free it when
 * the SecretKey is dropped -- pvw_sk_free clears the device copy (Zeroize + ZeroizeOnDrop, secret_key.rs:20-30).
 * sk: k x l coefficients on the host.  The handle belongs to `ctx` and must be freed before it. */
typedef struct pvw_sk pvw_sk;
PVW_API int32_t pvw_sk_load(pvw_ctx* ctx, const int64_t* sk /*[k][l]*/, pvw_sk** out);
/* The resident key pvw_sk_load(ctx, pvw_sample_secret_keys(sk_seed, party_index)) would hold, drawn on the device
 * (SecretKey::random, secret_key.rs:45-63; Party::new, public_key.rs:62-79): no coefficient buffer exists at any time.  Same
 * ownership and pvw_sk_free rules. */
PVW_API int32_t pvw_sk_load_seeded(pvw_ctx* ctx, const uint8_t sk_seed[32], uint32_t party_index, pvw_sk** out);
PVW_API int32_t pvw_sk_free(pvw_sk* key);
PVW_API int32_t pvw_decrypt_batch_device_sk(pvw_ctx* ctx, const pvw_sk* key, const uint64_t* d_c1s,
                                            const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                            uint64_t* d_noisy, uint64_t* d_out, void* stream);
/* ---- decrypt for every party: the loop over decrypt_party_shares (decryption.rs:281-325) that examples/pvw.rs:138-149 runs
 * for all parties and checks as results[recipient][dealer] (:157-170), as tests/crypto.rs:284-287 does; over a subset of
 * dealers (the "valid" ciphertexts) it is examples/pvw_valid_dec.rs:201-209.  Every party of [party_lo, party_hi) decrypts
 * its share of each of D dealer ciphertexts:
 *   out[p][d] = decode_scalar_pvw_rns( sum_j NTT(sk[p][j]) * c1s[d][j] - c2s[d][party_lo + p] )   (decryption.rs:257-274, :10-58)
 * sk [P][k][l] (P = party_hi - party_lo); c1s [D][k][L][l]; c2s [D][n][L][l] (whole ciphertexts, global party rows: the call
 * reads rows [party_lo, party_hi) of each and no other); out_u64 [P][D].  out[p][d] is the word pvw_decrypt_batch returns for
 * party p's key and column on the same input words, whatever they are.  Any D >= 1; in_repr POWER or NTT (POWER input is
 * transformed in scratch: the caller's buffers are only read).  Argument errors (InvalidParameters for NULL, D = 0, an empty
 * range or party_hi > n; InvalidFormat for in_repr) come before any device work.  The parties' s-hat rows and the dealers'
 * c1 meet in one digit GEMM on the matrix cores; fewer than 22 parties run the per-party kernels party by party.
 * Device scratch stays below about 4.5 GiB whatever P and D (dealers in groups of <= 128, parties in chunks); every
 * region derived from the keys (coefficients, tiled s-hat, GEMM intermediate, noisy polynomials) is cleared before the
 * call's work completes (pvw_selftest_secret_residue).  The host variant stages c1 and the c2 rows it needs in bounded
 * pieces; the device variant is asynchronous on `stream` like pvw_decrypt_batch_device. */
PVW_API int32_t pvw_decrypt_all(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, uint32_t in_repr,
                                uint64_t* out_u64);
PVW_API int32_t pvw_decrypt_all_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                       const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                       uint32_t in_repr, uint64_t* d_out, void* stream);
/* ---- checked decryption: each share's noise and whether its decode was lossy --------------------------
 * For a noisy polynomial z (power basis) let P be the decode's plaintext before the u64 conversion, centre(-z_0 - noise_0)
 * (decryption.rs:51-53).  Then residual_i = centre(-z_i - P Delta^i mod Q), i = 0 .. l-1, centre into (-Q/2, Q/2], and
 *   noise[d]  = min(max_i |residual_i|, 2^64 - 1)         (exact below 2^64 - 1, saturating above)
 *   status[d] = PVW_DEC_LOSSY when the returned word is not P (P < 0 or P >= 2^64: the conversion of :226-247 decided it,
 *               "small negative -> 0" included); every other bit 0
 *   out[d]    = the word the unchecked entry point returns on the same input words, bit for bit.
 * For an honest ciphertext residual is the decryption noise s e1 - e r - e2 (up to sign); for garbage noise saturates.
 * noise and status may each be NULL.  Every entry below extends the one it names and keeps its argument rules. */
enum { PVW_DEC_LOSSY = 1 };
/* extends pvw_decrypt_batch (host buffers): noise [D], status [D] */
PVW_API int32_t pvw_decrypt_batch_checked(pvw_ctx* ctx, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col,
                                          size_t num_dealers, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise,
                                          uint32_t* status);
/* extends pvw_decrypt_batch_device: d_noise [D], d_status [D] on the device */
PVW_API int32_t pvw_decrypt_batch_checked_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s,
                                                 const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                                 uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                                 void* stream);
/* extends pvw_decrypt_batch_device_sk */
PVW_API int32_t pvw_decrypt_batch_device_sk_checked(pvw_ctx* ctx, const pvw_sk* key, const uint64_t* d_c1s,
                                                    const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                                    uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                                    uint32_t* d_status, void* stream);
/* extend pvw_decrypt_all / pvw_decrypt_all_device: noise / status [P][D] like out (both sides of the 22-party dispatch) */
PVW_API int32_t pvw_decrypt_all_checked(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                        const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, uint32_t in_repr,
                                        uint64_t* out_u64, uint64_t* noise, uint32_t* status);
PVW_API int32_t pvw_decrypt_all_checked_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                               const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                               uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                               void* stream);
/* extends pvw_decode (host buffers, decode on the device) */
PVW_API int32_t pvw_decode_checked(pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64, uint64_t* noise,
                                   uint32_t* status);
/* extends pvw_decode_device */
PVW_API int32_t pvw_decode_checked_device(pvw_ctx* ctx, const uint64_t* d_noisy, size_t count, uint64_t* d_out,
                                          uint64_t* d_noise, uint32_t* d_status, void* stream);
/* extends pvw_decode_host: host big integers, residuals by the definition above (no GPU needed) */
PVW_API int32_t pvw_decode_checked_host(const pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64,
                                        uint64_t* noise, uint32_t* status);
/* extends pvw_selftest_decode_fixed: the fixed-width device decode with its report, run on the host (the recurrence
 * residual_{i+1} = Delta residual_i + tmp_i on the residues, one lift a step).  No product path calls it. */
PVW_API int32_t pvw_selftest_decode_checked(const pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64,
                                            uint64_t* noise, uint32_t* status);

/* ---- sums of dealers' ciphertexts: the scheme is additively homomorphic, so the component-wise sum of the valid
 * dealers' ciphertexts is a ciphertext of the sum of their shares under the same keys -- the step examples/pvw.rs:138-170 and
 * examples/pvw_valid_dec.rs:150-209 take on decrypted shares (party i's result is the sum over the valid dealers), taken
 * before the decrypt.  Nobody needs a key to fold; a party then needs one inner product and one decode instead of D.
 *   c1_out[j] = sum_{d valid} c1s[d][j],  c2_out[r - row_lo] = sum_{d valid} c2s[d][r]  (r in [row_lo, row_hi)), word by word mod q_i.
 * c1s [D][k][L][l]; c2s [D][n][L][l] (whole ciphertexts, global party rows: rows [row_lo, row_hi) are read and no other);
 * valid: uint8_t[D], dealer d is summed when valid[d] != 0, NULL = every dealer; *count (may be NULL) = dealers summed.
 * Element-wise, so PVW_REPR_POWER and PVW_REPR_NTT alike: all inputs in one representation, the output in the same (the call
 * does not transform).  Residue words as everywhere: any 64-bit input word, every output word below q_i.
 * Argument errors (InvalidParameters for NULL, D = 0, D >= 2^32, an empty row range, row_hi > n) come before any device work.
 * The noise of the result is the sum of the dealers' noises: pvw_ctx_sum_capacity says for how many dealers the decode is
 * PROVEN exact; no sum entry point refuses on noise grounds -- the checked decode of the aggregate reports its exact noise. */
/* device pointers, asynchronous on `stream`; d_valid is read when the kernel runs (a captured call replays with the mask of the
 * moment).  An all-zero mask writes zeros and *d_count = 0.  After pvw_prepare(PVW_PREPARE_SUM) on the stream the call neither
 * allocates nor synchronises; under stream capture without it: PVW_ERR_INVALID_PARAMETERS naming pvw_prepare, nothing enqueued. */
PVW_API int32_t pvw_ct_sum_device(pvw_ctx* ctx, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                  const uint8_t* d_valid, uint32_t row_lo, uint32_t row_hi, uint64_t* d_c1_out, uint64_t* d_c2_out,
                                  uint32_t* d_count, void* stream);
/* host buffers (synchronous): only the valid dealers are staged, in bounded pieces.  No valid dealer: PVW_ERR_INSUFFICIENT_DATA
 * before any device work. */
PVW_API int32_t pvw_ct_sum(pvw_ctx* ctx, const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                           uint32_t row_lo, uint32_t row_hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* count);
/* the same function in plain loops on the host cores (no GPU needed): what the device kernels are tested against */
PVW_API int32_t pvw_ct_sum_host(const pvw_ctx* ctx, const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers,
                                const uint8_t* valid, uint32_t row_lo, uint32_t row_hi, uint64_t* c1_out, uint64_t* c2_out,
                                uint32_t* count);
/* One party's aggregate share: the sum over (c1, the party's column c2col [D][L][l]) of the valid dealers, then the decrypt of
 * that ONE ciphertext (decryption.rs:257-274) and its checked decode (contract unchanged): out[1], noise[1] = the
 * exact max residual of the aggregate, status[1] = PVW_DEC_LOSSY when the sum of the plaintexts is not representable
 * (>= 2^64 or negative; pvw_decrypt_sum_plain* below return such a sum exactly, reduced or wide).  noise / status / count may be NULL.  d_noisy [L][l] (power basis) is an optional output (NULL: kept
 * in scratch and cleared).  in_repr POWER or NTT (the sum is transformed in scratch; the caller's buffers are only read).
 * Key hygiene as pvw_decrypt_batch*.  The device forms follow pvw_ct_sum_device's rules on pvw_prepare and stream capture. */
PVW_API int32_t pvw_decrypt_sum_checked_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                               size_t num_dealers, const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy,
                                               uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                               void* stream);
/* with a resident key (pvw_sk_load) */
PVW_API int32_t pvw_decrypt_sum_device_sk_checked(pvw_ctx* ctx, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                                  size_t num_dealers, const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy,
                                                  uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                                  void* stream);
/* host buffers; no valid dealer: PVW_ERR_INSUFFICIENT_DATA before any device work */
PVW_API int32_t pvw_decrypt_sum_checked(pvw_ctx* ctx, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col,
                                        size_t num_dealers, const uint8_t* valid, uint32_t in_repr, uint64_t* out_u64,
                                        uint64_t* noise, uint32_t* status, uint32_t* count);
/* Every party of [party_lo, party_hi) decrypts its aggregate share: the sum over c1 and rows [party_lo, party_hi) of c2, then
 * pvw_decrypt_all_checked's machinery on that ONE ciphertext.  sk [P][k][l]; c1s [D][k][L][l]; c2s [D][n][L][l]; out / noise /
 * status [P].  Argument rules of pvw_decrypt_all plus those of pvw_ct_sum. */
PVW_API int32_t pvw_decrypt_all_sum_checked(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                            const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                                            uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint32_t* count);
PVW_API int32_t pvw_decrypt_all_sum_checked_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                                   const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                                   const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise,
                                                   uint32_t* d_status, uint32_t* d_count, void* stream);
/* Advisory, host only: *max_dealers = floor(R / noise_bound) (saturated to u64), R the largest integer with
 * R (Delta^(l-1) + 1) < Q / 2.  max_i |noise_i| <= R is SUFFICIENT for the gadget decode to be exact (every intermediate of
 * decryption.rs:10-58 stays below Q/2 in magnitude); it is not necessary, and honest noise is far below pvw_ctx_noise_bound.
 * The reference's gate (parameters.rs:510-551) is not a decoding radius and promises nothing about an aggregate. */
PVW_API int32_t pvw_ctx_sum_capacity(const pvw_ctx* ctx, uint64_t* max_dealers);

/* ---- plain-modulus decode: exact shares and aggregates beyond 64 bits -----------------------------------
 * PVSS shares live in Z_p, and a party wants sum_d share_d mod p; the u64 conversion at the end of the reference's decode
 * (extract_constant_term_as_u64, decryption.rs:226-247) returns 0 once the recovered plaintext P leaves [0, 2^64), which the
 * sum of sixteen 61-bit shares does.  These entry points finish the decode in the caller's modulus, or hand back the wide
 * integer, on the device, in the launch that ran the chain.  P is 8.6's P: the centred plaintext before the conversion.
 * Each entry is the checked one it names plus the plain options, three trailing arguments (a pvw_plain_t, flattened so that
 * every argument keeps a fixed-width C type):
 *   plain_modulus  0 = none; else 2 <= plain_modulus < 2^62, ANY integer (even, a power of two, composite):
 *                  out[d] = P mod plain_modulus, the mathematical residue in [0, plain_modulus) -- P = -5 gives modulus - 5.
 *                  0: out[d] is the word the checked entry point returns, bit for bit.
 *   wide_words     0 = none; else 1 .. W, W = the 64-bit words of Q: wide[d] receives the low wide_words words of |P|.
 *   wide           [count][wide_words], little-endian magnitude of P, laid out like out (so [P][D][wide_words] for
 *                  pvw_decrypt_all_plain*); a device pointer in the *_device forms.
 * noise[d] keeps its 8.6 definition.  status[d]: PVW_DEC_LOSSY keeps its meaning exactly ("the plain u64 entry point's word
 * would not be P" -- informational here, out is exact regardless); PVW_DEC_NEGATIVE: P < 0; PVW_DEC_WIDE_TRUNCATED: |P| does
 * not fit wide_words words (never set when wide_words == 0).  Only these entry points set the two new bits.
 * Argument errors, PVW_ERR_INVALID_PARAMETERS before any device work: plain_modulus 1 or >= 2^62; wide_words > W;
 * wide_words != 0 with wide NULL.  plain_modulus = 0 and wide_words = 0 make a call identical to the checked call it extends.
 * Input side: encrypt still takes u64 scalars read as i64 (encryption.rs:195), so a share must be below 2^63 to mean itself;
 * reduced shares with p < 2^62 always are, and a share encoded as a negative i64 comes back as its residue.
 * Radius: the result is exact whenever the noise is inside the decoding radius pvw_ctx_sum_capacity describes; |P| itself
 * only has to stay below Q/2 (tmp_i = z_i Delta - z_{i+1} cancels P exactly mod Q, so the noise chain does not depend on P).
 * Key hygiene, pvw_prepare(PVW_PREPARE_SUM) and stream-capture rules are those of the call each one extends; the scratch
 * pvw_prepare fixes covers wide at wide_words = W.  The options travel by value into the launch: a captured call replays
 * with them. */
typedef struct {
  uint64_t modulus;     /* 0 = none; else 2 <= modulus < 2^62 */
  uint32_t wide_words;  /* 0 = none; else 1 .. W */
  uint64_t* wide;       /* [count][wide_words] */
} pvw_plain_t;          /* the three trailing arguments below, as one value (host/pvw.hpp carries them so) */
enum { PVW_DEC_NEGATIVE = 2, PVW_DEC_WIDE_TRUNCATED = 4 };
PVW_API int32_t pvw_decode_plain(pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64, uint64_t* noise,
                                 uint32_t* status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide);
PVW_API int32_t pvw_decode_plain_device(pvw_ctx* ctx, const uint64_t* d_noisy, size_t count, uint64_t* d_out,
                                        uint64_t* d_noise, uint32_t* d_status, uint64_t plain_modulus, uint32_t wide_words,
                                        uint64_t* d_wide, void* stream);
/* host big integers, by the definition (no GPU needed) */
PVW_API int32_t pvw_decode_plain_host(const pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64,
                                      uint64_t* noise, uint32_t* status, uint64_t plain_modulus, uint32_t wide_words,
                                      uint64_t* wide);
/* SELF-TEST: the fixed-width device algorithm with the plain tail, run on the host.  No product path calls it. */
PVW_API int32_t pvw_selftest_decode_plain(const pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64,
                                          uint64_t* noise, uint32_t* status, uint64_t plain_modulus, uint32_t wide_words,
                                          uint64_t* wide);
PVW_API int32_t pvw_decrypt_batch_plain(pvw_ctx* ctx, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col,
                                        size_t num_dealers, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise,
                                        uint32_t* status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide);
PVW_API int32_t pvw_decrypt_batch_plain_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s,
                                               const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                               uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                               uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
PVW_API int32_t pvw_decrypt_batch_device_sk_plain(pvw_ctx* ctx, const pvw_sk* key, const uint64_t* d_c1s,
                                                  const uint64_t* d_c2col, size_t num_dealers, uint32_t in_repr,
                                                  uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                                  uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
/* wide [P][D][wide_words], inside the regions the call marks secret and clears */
PVW_API int32_t pvw_decrypt_all_plain(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                      const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, uint32_t in_repr,
                                      uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint64_t plain_modulus,
                                      uint32_t wide_words, uint64_t* wide);
PVW_API int32_t pvw_decrypt_all_plain_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                             const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                             uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                             uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
/* the aggregate share in Z_p: out[0] = (sum over the valid dealers of the party's shares) mod plain_modulus, wide [1][wide_words] */
PVW_API int32_t pvw_decrypt_sum_plain(pvw_ctx* ctx, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col,
                                      size_t num_dealers, const uint8_t* valid, uint32_t in_repr, uint64_t* out_u64,
                                      uint64_t* noise, uint32_t* status, uint32_t* count, uint64_t plain_modulus,
                                      uint32_t wide_words, uint64_t* wide);
PVW_API int32_t pvw_decrypt_sum_plain_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                             size_t num_dealers, const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy,
                                             uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                             uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
PVW_API int32_t pvw_decrypt_sum_device_sk_plain(pvw_ctx* ctx, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                                size_t num_dealers, const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy,
                                                uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                                uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
/* out / noise / status [P], wide [P][wide_words] */
PVW_API int32_t pvw_decrypt_all_sum_plain(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                          const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                                          uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint32_t* count,
                                          uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide);
PVW_API int32_t pvw_decrypt_all_sum_plain_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                                 const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                                 const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise,
                                                 uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus,
                                                 uint32_t wide_words, uint64_t* d_wide, void* stream);

/* ---- weighted sums of dealers' ciphertexts: the scheme is linear, not just additive, so sum_d w_d ct_d is a
 * ciphertext of sum_d w_d m_d under the same keys, with noise sum_d |w_d| noise_d.  With w the Lagrange weights at 0 of the valid
 * old holders (pvw_shamir_lagrange_weights) a committee handover -- every old holder d re-shares its share with a fresh polynomial
 * f_d, new party j needs sum_d lambda_d f_d(j + 1) mod p -- is one pass over the ciphertexts and ONE decrypt per party instead of
 * D; w = -1 gives differences, small random weights batch checks.  Each function takes the arguments of the pvw_ct_sum /
 * pvw_decrypt_sum_plain call it mirrors plus `weights` directly after `valid`, and keeps that call's contract with this changed:
 *   out = sum_{d participating} w_d in_d, word by word mod q_i.  weights: int64_t[D], w_d ANY value (INT64_MIN included) read as
 *   the integer it is (its residue mod q_i is ((w mod q_i) + q_i) mod q_i); NULL: PVW_ERR_INVALID_PARAMETERS "NULL argument".
 *   Dealer d PARTICIPATES when it is valid (valid == NULL or valid[d] != 0) and w_d != 0; a dealer that does not is never read.
 *   *count = participating dealers.  Any 64-bit input word, every output word below q_i; both representations; the row range of
 *   pvw_ct_sum.  With every weight 1 each call is bit-equal to the pvw_ct_sum* / pvw_decrypt_*sum_plain* call it mirrors.
 * Argument errors are those of the mirrored call and come before any device work. */
/* device pointers (d_weights too), asynchronous on `stream`; mask AND weights are read when the kernel runs, so a captured call
 * replays with the values of the moment.  An all-zero mask or all-zero weights write zeros and *d_count = 0.  pvw_prepare
 * (PVW_PREPARE_SUM) and stream capture exactly as pvw_ct_sum_device, with the same scratch. */
PVW_API int32_t pvw_ct_lincomb_device(pvw_ctx* ctx, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                      const uint8_t* d_valid, const int64_t* d_weights, uint32_t row_lo, uint32_t row_hi,
                                      uint64_t* d_c1_out, uint64_t* d_c2_out, uint32_t* d_count, void* stream);
/* host buffers (synchronous): only the participating dealers are staged, in bounded pieces, each piece with its weights.  No
 * participating dealer: PVW_ERR_INSUFFICIENT_DATA before any device work. */
PVW_API int32_t pvw_ct_lincomb(pvw_ctx* ctx, const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                               const int64_t* weights, uint32_t row_lo, uint32_t row_hi, uint64_t* c1_out, uint64_t* c2_out,
                               uint32_t* count);
/* the definition in plain loops on the host cores (no GPU needed): what the device kernels are tested against */
PVW_API int32_t pvw_ct_lincomb_host(const pvw_ctx* ctx, const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers,
                                    const uint8_t* valid, const int64_t* weights, uint32_t row_lo, uint32_t row_hi, uint64_t* c1_out,
                                    uint64_t* c2_out, uint32_t* count);
/* One party's view of the combination (c1 plus the party's column): pvw_decrypt_sum_plain* with the sum replaced.  plain_modulus /
 * wide_words / wide, the status bits, key hygiene and the capture rules are unchanged; both options 0: the checked word.
 * The `noise` word saturates at 2^64 - 1, which a combination with field-sized weights always reaches (its noise is near
 * 2^72): for such combinations pvw_ctx_lincomb_fits below, not the noise word, is what a caller has. */
PVW_API int32_t pvw_decrypt_lincomb_plain(pvw_ctx* ctx, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col,
                                          size_t num_dealers, const uint8_t* valid, const int64_t* weights, uint32_t in_repr,
                                          uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint32_t* count,
                                          uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide);
PVW_API int32_t pvw_decrypt_lincomb_plain_device(pvw_ctx* ctx, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                                 size_t num_dealers, const uint8_t* d_valid, const int64_t* d_weights,
                                                 uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                                 uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus, uint32_t wide_words,
                                                 uint64_t* d_wide, void* stream);
PVW_API int32_t pvw_decrypt_lincomb_device_sk_plain(pvw_ctx* ctx, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                                    size_t num_dealers, const uint8_t* d_valid, const int64_t* d_weights,
                                                    uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                                    uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus,
                                                    uint32_t wide_words, uint64_t* d_wide, void* stream);
/* Every party of [party_lo, party_hi): pvw_decrypt_all_sum_plain* with the combination.  out / noise / status [P], wide [P][wide_words].
 * The handover: secrets = the old shares sigma_d = F(d + 1) into pvw_deal_shares; valid = the old holders whose dealing verified;
 * weights = pvw_shamir_lagrange_weights over the valid old indices (0 elsewhere); plain_modulus = p.  out[j] is new party j's share
 * of F(0). */
PVW_API int32_t pvw_decrypt_all_lincomb_plain(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                              const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                                              const int64_t* weights, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise,
                                              uint32_t* status, uint32_t* count, uint64_t plain_modulus, uint32_t wide_words,
                                              uint64_t* wide);
PVW_API int32_t pvw_decrypt_all_lincomb_plain_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                                     const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                                     const uint8_t* d_valid, const int64_t* d_weights, uint32_t in_repr,
                                                     uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                                     uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
/* Advisory, host only (host big integers): *fits = 1 iff (sum over the participating dealers of |w_d|) * pvw_ctx_noise_bound <= R,
 * R the radius pvw_ctx_sum_capacity is built on; else 0.  Sufficient, not necessary, like that function, and no entry point refuses
 * on noise grounds.  weights / valid are HOST pointers (valid may be NULL). */
PVW_API int32_t pvw_ctx_lincomb_fits(const pvw_ctx* ctx, const int64_t* weights, size_t num_dealers, const uint8_t* valid,
                                     uint32_t* fits);
/* Host only, no context: weights_out[i] = the Lagrange weight at 0 of the point indices[i] + 1 among the points indices[.] + 1,
 * mod p = plain_modulus, CENTRED in (-p/2, p/2] (so that it enlarges the noise as little as its residue class allows).  The routine
 * and the argument rules of pvw_shamir_reconstruct below: p prime and < 2^62, no duplicate index, every index < p - 1, count >= 1. */
PVW_API int32_t pvw_shamir_lagrange_weights(uint64_t plain_modulus, const uint64_t* indices, size_t count, int64_t* weights_out);

/* ---- many weighted sums of the same dealers' ciphertexts in one pass: R = num_combos rows of weights over one set
 * of D ciphertexts -- the handover of a PACKED sharing (one row per slot: the Lagrange weights at the point -m of the valid old
 * points), batched random-combination checks, the re-dealt polynomials' values at several points.  weights: int64_t [R][D], row-major,
 * each row under the per-weight rules above.  Dealer d PARTICIPATES IN COMBINATION r when it is valid and weights[r][d] != 0;
 * counts[r] (may be NULL) is the number of such dealers.  A dealer that is not valid, or whose weight is 0 in every row, is never
 * read.  Results: c1_out [R][k][L][l], c2_out [R][row_hi - row_lo][L][l]; row r is, bit for bit on every word and on counts[r], what
 * the pvw_ct_lincomb* call of the same form returns with weights + r * D (any 64-bit input word, both representations); a row with no
 * participant is all zeros with counts[r] = 0, in every form.  num_combos = 1 is that call, through its kernel.  Each ciphertext is
 * read once per tile of rows, and crosses the bus once in the host-buffer forms.
 * Refused with PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the mirrored pvw_ct_lincomb* /
 * pvw_decrypt_all_lincomb_plain* call refuses, with its text; num_combos = 0; on the device forms num_combos >= 2^31.  The host-buffer
 * forms return PVW_ERR_INSUFFICIENT_DATA only when no dealer participates in ANY row. */
/* Host only, no context: weights_out [num_targets][count]; row j = the Lagrange weights AT the point (targets[j] + 1) mod p of the
 * points indices[i] + 1, centred in (-p/2, p/2].  targets[j] < p (p - 1 is the point 0: that row equals
 * pvw_shamir_lagrange_weights; p - 1 - m is the point -m).  A target that is one of the indices gives that unit vector.
 * Duplicate targets allowed.  Otherwise the rules of pvw_shamir_lagrange_weights, plus NULL targets / num_targets = 0 refused. */
PVW_API int32_t pvw_shamir_lagrange_weights_at(uint64_t plain_modulus, const uint64_t* indices, size_t count, const uint64_t* targets,
                                               size_t num_targets, int64_t* weights_out);
/* the definition in plain loops on the host cores (no GPU needed): the loop of pvw_ct_lincomb_host over the rows */
PVW_API int32_t pvw_ct_lincomb_many_host(const pvw_ctx* ctx, const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers,
                                         const uint8_t* valid, const int64_t* weights, size_t num_combos, uint32_t row_lo,
                                         uint32_t row_hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* counts);
/* device pointers (d_weights [R][D] and d_counts [R] too), asynchronous on `stream`, straight into the caller's buffers; mask and
 * weights are read when the kernels run.  pvw_prepare(PVW_PREPARE_SUM) and stream capture exactly as pvw_ct_lincomb_device. */
PVW_API int32_t pvw_ct_lincomb_many_device(pvw_ctx* ctx, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                           const uint8_t* d_valid, const int64_t* d_weights, size_t num_combos, uint32_t row_lo,
                                           uint32_t row_hi, uint64_t* d_c1_out, uint64_t* d_c2_out, uint32_t* d_counts, void* stream);
/* host buffers (synchronous): a dealer is staged when it participates in at least one row */
PVW_API int32_t pvw_ct_lincomb_many(pvw_ctx* ctx, const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                                    const int64_t* weights, size_t num_combos, uint32_t row_lo, uint32_t row_hi, uint64_t* c1_out,
                                    uint64_t* c2_out, uint32_t* counts);
/* pvw_decrypt_all_lincomb_plain[_device] with `num_combos` directly after the weights and `counts` [R] in place of `count`:
 * out / noise / status [P][R], wide [P][R][wide_words] -- the [party][dealer] layout of pvw_decrypt_all* with the combinations in the
 * dealers' place, so strides (1, R) feed pvw_shamir_reconstruct_checked* in place.  Column r equals the num_combos = 1 call.  The
 * combined ciphertexts (public) live in the stream's scratch and ONE decrypt of all of them follows.  Under stream capture the
 * device form needs that scratch sized already: by an earlier call on that stream OUTSIDE capture with the same party range and at
 * least as many combinations; otherwise PVW_ERR_INVALID_PARAMETERS with nothing enqueued (pvw_prepare does not size it).
 * The packed handover: weights = pvw_shamir_lagrange_weights_at over the valid old indices with targets p - 1 - m, m < K (0 at the
 * other dealers); out[j][m] is new party j's share of secret m. */
PVW_API int32_t pvw_decrypt_all_lincomb_many_plain_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                                          const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                                          const uint8_t* d_valid, const int64_t* d_weights, size_t num_combos,
                                                          uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                                          uint32_t* d_counts, uint64_t plain_modulus, uint32_t wide_words,
                                                          uint64_t* d_wide, void* stream);
PVW_API int32_t pvw_decrypt_all_lincomb_many_plain(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk,
                                                   const uint64_t* c1s, const uint64_t* c2s, size_t num_dealers, const uint8_t* valid,
                                                   const int64_t* weights, size_t num_combos, uint32_t in_repr, uint64_t* out_u64,
                                                   uint64_t* noise, uint32_t* status, uint32_t* counts, uint64_t plain_modulus,
                                                   uint32_t wide_words, uint64_t* wide);

/* ---- the one-word handover in one call, its weights from a mask that may be made on the device -----------------
 * weights [num_targets][num_holders], row-major: row j = the Lagrange weights AT the point (targets[j] + 1) mod p (the target rule of
 * pvw_shamir_lagrange_weights_at: p - 1 is the point 0, p - 1 - m the point -m) over the points indices[d] + 1 of the holders with
 * valid[d] != 0 (valid == NULL: all of them), centred in (-p/2, p/2]; the column of a holder that is not valid is 0.  Row j is, bit
 * for bit, pvw_shamir_lagrange_weights_at over the compacted valid indices, scattered back to their columns.  targets == NULL is the
 * single point 0 and num_targets must then be 1.  A target on a VALID holder's point gives that holder's unit vector; a target on a
 * holder that is not valid is an ordinary point.  *count (may be NULL) = the number of valid holders; with none, every weight is 0
 * and the count is 0, which is no error (as pvw_ct_lincomb_device with an all-zero mask).
 * Refused with PVW_ERR_INVALID_PARAMETERS before any device work, nothing written, and the same by both forms: NULL indices or
 * weights; num_holders = 0; num_targets = 0; what pvw_shamir_lagrange_weights refuses (p not prime or >= 2^62, a duplicate index, an
 * index >= p - 1) about ALL num_holders indices, masked ones included -- the device form cannot know the mask at call time, and the
 * host form follows it; a target >= p; on the device num_holders >= 2^32 or num_targets >= 2^31. */
PVW_API int32_t pvw_shamir_handover_weights_host(uint64_t plain_modulus, const uint64_t* indices, const uint8_t* valid, size_t num_holders,
                                                 const uint64_t* targets, size_t num_targets, int64_t* weights, uint32_t* count);
/* indices and targets are HOST arrays, consumed at call time (they travel as kernel arguments); d_valid, d_weights and d_count are
 * DEVICE pointers, and the mask is read when the kernels run: a captured call replays with the mask of the moment.  Asynchronous on
 * `stream`; allocates nothing once the stream's workspace holds the call's public matrices, which it sizes by (num_holders,
 * num_targets).  Under stream capture that block must be there already, from an earlier call on that stream OUTSIDE capture with at
 * least as many holders and targets; otherwise PVW_ERR_INVALID_PARAMETERS with nothing enqueued. */
PVW_API int32_t pvw_shamir_handover_weights_device(pvw_ctx* ctx, uint64_t plain_modulus, const uint64_t* indices, const uint8_t* d_valid,
                                                   size_t num_holders, const uint64_t* targets, size_t num_targets, int64_t* d_weights,
                                                   uint32_t* d_count, void* stream);
/* The holder mask from a report: valid_out[c] = 1 iff for no row r the element at r * row_stride + c * col_stride has
 * status & status_bits != 0 or noise > noise_bound, else 0; *num_valid (may be NULL) = the number of ones.  Either array may be NULL,
 * not both; both are only read.  The argument and refusal rules of pvw_shamir_erasure_mask_* (count, rows, strides of 0).  With
 * rows = 1, strides (count, 1), status = the col_err of a corrected reconstruction and status_bits = 0xFFFFFFFF: the columns without
 * a wrong share.  With strides (D, 1): the [party][dealer] report of pvw_decrypt_all_*_checked / _plain in place.  The device form
 * takes device pointers throughout, is asynchronous on `stream`, and on the device count and rows are below 2^31; under stream
 * capture the stream's workspace must exist (any earlier call of this section on that stream). */
PVW_API int32_t pvw_shamir_valid_mask_host(uint32_t* status, const uint64_t* noise, uint32_t status_bits, uint64_t noise_bound, size_t count,
                                           size_t rows, size_t row_stride, size_t col_stride, uint8_t* valid_out, uint32_t* num_valid);
PVW_API int32_t pvw_shamir_valid_mask_device(pvw_ctx* ctx, uint32_t* d_status, const uint64_t* d_noise, uint32_t status_bits,
                                             uint64_t noise_bound, size_t count, size_t rows, size_t row_stride, size_t col_stride,
                                             uint8_t* d_valid_out, uint32_t* d_num_valid, void* stream);
/* Every new party's new share in one call: pvw_decrypt_all_lincomb_many_plain[_device] with (indices, targets, num_targets) in place
 * of (weights, num_combos) and one `count` word, the number of valid holders, in place of `counts`.  plain_modulus is the field of
 * the weights (prime, below 2^62) AND the decode modulus.  out / noise / status [P][T], wide [P][T][wide_words].  Behind the checks:
 * the weights above, the many-combinations call itself with valid = NULL there (a masked holder's weights are 0, so its ciphertext
 * is never addressed), and that call's report as it is.  Results are bit for bit pvw_shamir_handover_weights_host ->
 * pvw_decrypt_all_lincomb_many_plain with the same arguments.  Refused: what the weights refuse, then what that call refuses.
 * Nothing refuses on noise grounds: pvw_ctx_lincomb_fits stays the advisory test.  Keys are staged, marked and wiped by the
 * many-combinations call.
 * Device form: d_valid is a DEVICE pointer (NULL: all valid), indices and targets HOST arrays consumed at call time; asynchronous on
 * `stream`.  With no valid holder: zeros and *d_count = 0.  Under stream capture every workspace block (the weights' public
 * matrices, the weight rows, the many-combinations scratch) must be sized by an earlier call on that stream OUTSIDE capture with the
 * same party range and at least as many holders and targets; otherwise PVW_ERR_INVALID_PARAMETERS with nothing enqueued.  A replay
 * reads no host memory and follows the mask of the moment.
 * Host-buffer form (synchronous): valid is a HOST array, only valid holders are staged (in pieces, as the many-combinations call
 * stages them); the weights run through the same kernels on a pooled workspace, so the call joins the concurrency promise.  With
 * no valid holder: PVW_ERR_INSUFFICIENT_DATA. */
PVW_API int32_t pvw_decrypt_all_handover_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                                const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_holders, const uint8_t* d_valid,
                                                const uint64_t* indices, const uint64_t* targets, size_t num_targets, uint32_t in_repr,
                                                uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                                uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream);
PVW_API int32_t pvw_decrypt_all_handover(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk, const uint64_t* c1s,
                                         const uint64_t* c2s, size_t num_holders, const uint8_t* valid, const uint64_t* indices,
                                         const uint64_t* targets, size_t num_targets, uint32_t in_repr, uint64_t* out_u64,
                                         uint64_t* noise, uint32_t* status, uint32_t* count, uint64_t plain_modulus,
                                         uint32_t wide_words, uint64_t* wide);

/* ---- Shamir shares: from secrets to ciphertexts in one call, and back --------------------------------------
 * The dealing end of the protocol the reference's examples sketch (examples/pvw.rs:95-131 fill the share matrix with arbitrary
 * numbers; the reference has no sharing code, so this contract is the library's own).  All arithmetic in Z_p, p = plain_modulus:
 *   p prime, n < p < 2^62 (the points 1..n and their differences must be invertible); primality is checked on the host with a
 *   deterministic Miller-Rabin.  A composite p, p <= n, p >= 2^62: PVW_ERR_INVALID_PARAMETERS before any device work; so are
 *   degree >= n, num_dealers = 0 and NULL arguments.
 *   f_d(x) = s_d + a_{d,1} x + ... + a_{d,t} x^t mod p (t = degree, 0 <= t <= n - 1); shares[d][i] = f_d(i + 1) in [0, p) for the
 *   global party index i: any t + 1 shares determine s_d.  secrets [D] and explicit coefficients are words that mean w mod p (any
 *   word is accepted).  t = 0 copies the secret to every party and draws nothing.
 *   a_{d,j} (j = 1..t) = the first accepted draw of its own ChaCha8 stream: key = dealer d's 32-byte seed (seeds + 32 d, the
 *   seed pvw_encrypt_multi takes for that dealer), stream id (PVW_DOM_SHAMIR << 32) | j, draws next_u64() >> clz(p) accepted when
 *   < p.  coeffs != NULL ([D][t] words) replaces the draw (seeds may then be NULL).
 * shares [D][n]: the host routine writes every column; the device routines write columns [party_lo, party_hi) of a sharded
 * context and leave the others untouched. */
/* the contract in plain C++ on the host cores (no GPU needed): what the kernel is tested against */
PVW_API int32_t pvw_shamir_shares_host(const pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                       uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out);
/* device pointers (seeds stays a HOST pointer), asynchronous on `stream`; allocates nothing and may be captured */
PVW_API int32_t pvw_shamir_shares_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                         uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs, uint64_t* d_shares,
                                         void* stream);
/* host buffers (synchronous); the staged secrets, coefficients and shares are cleared before the call returns */
PVW_API int32_t pvw_shamir_shares(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                  uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out);
/* Deal: the shares are made on the device and encrypted in the same call -- neither they nor the coefficients exist on the host.
 *   pvw_deal_shares*(secrets, D, degree, p, seeds, ...)  ==  pvw_encrypt_multi*(shares, D, n, seeds, ...) bit for bit, with
 *   shares = pvw_shamir_shares_host(secrets, D, degree, p, seeds, NULL): both representations, both sides of the dealer-count
 *   dispatch, sharded contexts.  The arguments, checks and buffer layouts of the pvw_encrypt_multi* call each one extends (those
 *   checks come first, then the ones above).  _rs forms: dealer d's key is call_seed(S, c + d), derived when the kernels run;
 *   afterwards the state holds c + D, exactly as pvw_encrypt_multi_rs*.
 * The shares live in workspace scratch of a fixed size (one pass of dealers, [128][n] words) built together with the digit buffers:
 * pvw_prepare(PVW_PREPARE_MFMA) covers it, after which the *_device forms neither allocate nor synchronise and may be captured
 * (every replay of the _rs form deals a fresh sharing); under stream capture without it: the error of pvw_encrypt_multi_device,
 * nothing enqueued.  The scratch (and the uploaded secrets of the host-buffer forms) is cleared behind the call's last launch
 * (pvw_selftest_secret_residue). */
PVW_API int32_t pvw_deal_shares(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree, uint64_t plain_modulus,
                                const uint8_t* seeds /*[D][32]*/, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                       uint64_t plain_modulus, const uint8_t* seeds, uint64_t* d_c1, uint64_t* d_c2,
                                       uint32_t out_repr, void* stream);
PVW_API int32_t pvw_deal_shares_rs(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                   uint64_t plain_modulus, void* st, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_rs_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                          uint64_t plain_modulus, void* st, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr,
                                          void* stream);
/* Reconstruction, host only (no GPU, no context: t + 1 values per secret, and the combining party is not the dealer):
 *   out[s] = sum_i shares[s][i] * w_i mod p, w_i the Lagrange weights at 0 of the points indices[i] + 1, computed once.
 * indices [count]: global party indices; shares [num_secrets][count] (any words, read mod p).  count = 0, duplicate indices, an
 * index >= p - 1, a composite p or p >= 2^62: PVW_ERR_INVALID_PARAMETERS.  count must be at least degree + 1 for the result to
 * be the secret; the routine cannot know the degree and does not check. */
PVW_API int32_t pvw_shamir_reconstruct(uint64_t plain_modulus, const uint64_t* indices, const uint64_t* shares, size_t count,
                                       size_t num_secrets, uint64_t* out);
/* Checked reconstruction: the secrets AND a report on the shares they came from.  The reference leaves validity
 * of the shares "external" (examples/pvw_valid_dec.rs:150-159), so this contract is the library's own.  All arithmetic in Z_p,
 * p = plain_modulus prime and below 2^62.
 *   degree = t.  indices [count]: distinct global party indices, each < p - 1 (the points are x_c = indices[c] + 1); a HOST
 *   pointer in every form.  shares: num_secrets rows, element (s, c) at shares[s * secret_stride + c * point_stride] (strides in
 *   elements; any word, read mod p): strides (count, 1) read the [secret][party] rows of pvw_shamir_shares*, strides (1, D) the
 *   [party][dealer] result of pvw_decrypt_all* with every dealer a secret.
 *   Basis: columns 0..t in the caller's order; extras: columns t+1..count-1.  F_s: the polynomial of degree <= t through the
 *   basis points of secret s.
 *   out [num_secrets] = F_s(0).  bad [num_secrets] (or NULL): how many extras c have share(s, c) mod p != F_s(x_c).
 *   col_bad [count] (or NULL): for each column, how many secrets deviate there; 0 for the basis columns.
 * What the counts mean:
 *   one wrong extra share is flagged at exactly that (s, c), and out is right;
 *   one wrong basis share of secret s makes out[s] wrong and flags EVERY extra of s (the deviation at x_c is delta L_j(x_c), and
 *   L_j(x_c) != 0 outside the basis).  So a col_bad with one full column names a bad extra party; a col_bad with every extra
 *   column nonzero says the basis holds a bad party, and the caller reorders.  The routine detects; it neither corrects errors
 *   nor searches for a basis.
 * PVW_ERR_INVALID_PARAMETERS before any device work: NULL indices / shares / out (or ctx), num_secrets = 0, count < degree + 1,
 * duplicate indices, an index >= p - 1, a composite p or p >= 2^62, a stride of 0 (and, on the device, count or num_secrets
 * >= 2^31). */
/* the contract in plain C++ on the host cores (no context, no GPU): what the kernels are tested against */
PVW_API int32_t pvw_shamir_reconstruct_checked_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                    const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                    size_t point_stride, uint64_t* out, uint32_t* bad, uint32_t* col_bad);
/* device pointers (indices stays a HOST pointer, read before the call returns), asynchronous on `stream`.  The weight matrix
 * [t+1][count-t] lives in the stream's workspace, sized by the call: under stream capture the call needs an earlier call with the
 * same (degree, count) on that stream outside capture; without it: the error of pvw_encrypt_multi_device, nothing enqueued. */
PVW_API int32_t pvw_shamir_reconstruct_checked_device(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                      size_t count, const uint64_t* d_shares, size_t num_secrets,
                                                      size_t secret_stride, size_t point_stride, uint64_t* d_out, uint32_t* d_bad,
                                                      uint32_t* d_col_bad, void* stream);
/* host buffers (synchronous); the staged shares and secrets are cleared before the call returns */
PVW_API int32_t pvw_shamir_reconstruct_checked(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                               size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                               size_t point_stride, uint64_t* out, uint32_t* bad, uint32_t* col_bad);
/* Corrected reconstruction: the secrets although some shares are wrong, and which shares those are.  The shares of
 * one secret are a Reed-Solomon codeword of length count and dimension t + 1.  Write r = count - t - 1 (the redundant columns)
 * and E = r / 2 (rounded down).  Arguments as the checked calls; the contract is the library's own (the reference has none).
 *   Secret s is DECODABLE iff some polynomial F_s of degree <= t disagrees with row s (read mod p) in at most E columns; that
 *   F_s is then unique.
 *   decodable:   out[s] = F_s(0); nerr[s] = the number of disagreeing columns; bit c % 64 of err_mask[s * W + c / 64]
 *                (W = ceil(count / 64)) is set exactly for them; col_err[c] counts the decodable secrets that disagree in column c.
 *   undecodable: out[s] = 0, nerr[s] = PVW_SHAMIR_UNDECODABLE, its mask row is 0, and it adds nothing to col_err.
 *   nerr [num_secrets], col_err [count] and err_mask [num_secrets][W] may each be NULL.
 *   r = 0 is plain interpolation through all columns; r = 1 detects only (E = 0: one wrong share makes the secret undecodable).
 *   No column is a basis: a wrong share in any column is corrected alike, and the order of the columns changes no output
 *   (mask bits and col_err move with their columns).
 *   Every output is a function of the inputs alone, and the three forms agree bit for bit -- also for a p so small that a row
 *   with more than E wrong shares lies within E of ANOTHER polynomial: the row is decodable by the definition above, to that one.
 * The corrected share values, and F_s at any other point: pvw_shamir_evaluate_corrected* below.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: as the checked calls; on the device also
 * E + 1 > 4096 (count - degree - 1 >= 8192). */
#define PVW_SHAMIR_UNDECODABLE 0xFFFFFFFFu
/* the contract in plain C++ on the host cores (no context, no GPU), by Berlekamp-Welch and Gaussian elimination (cubic in count
 * per secret): what the kernels are tested against */
PVW_API int32_t pvw_shamir_reconstruct_corrected_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                      const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                      size_t point_stride, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                                      uint64_t* err_mask);
/* device pointers (indices stays a HOST pointer, read before the call returns), asynchronous on `stream`.  The scratch (two public
 * matrices [count][r] and [E+1][count], and per secret in flight r syndromes, E + 1 locator coefficients and count locator
 * values) lives in the stream's workspace, sized by the call: under stream capture the call needs an earlier call with the same
 * (degree, count) and at least as many secrets on that stream outside capture; without it: the error of
 * pvw_shamir_reconstruct_checked_device there, nothing enqueued.  The locator values are cleared behind the call's last launch. */
PVW_API int32_t pvw_shamir_reconstruct_corrected_device(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                        size_t count, const uint64_t* d_shares, size_t num_secrets,
                                                        size_t secret_stride, size_t point_stride, uint64_t* d_out, uint32_t* d_nerr,
                                                        uint32_t* d_col_err, uint64_t* d_err_mask, void* stream);
/* host buffers (synchronous); the staged shares and secrets are cleared before the call returns.  Covered by the concurrency
 * promise above (tests/test_gpu_shamir_evaluate.py runs it next to pvw_shamir_evaluate_corrected). */
PVW_API int32_t pvw_shamir_reconstruct_corrected(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                 size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                 size_t point_stride, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                                 uint64_t* err_mask);
/* Share repair: the corrected polynomials at any points.  The arguments of the corrected calls and their four
 * outputs, and behind point_stride: targets [num_targets] (a HOST array in every form, like indices; global party indices, the
 * point of target j is targets[j] + 1) and values [num_secrets][num_targets] (dense, row-major).  out may be NULL here as well;
 * values may not.
 *   Decodability, F_s, out, nerr, col_err and err_mask are those of the corrected calls, bit for bit: one decode yields every report.
 *   decodable:   values[s][j] = F_s(targets[j] + 1) mod p.     undecodable: the row of values is all 0.
 *   A target may be one of the indices: at a column the decode found right the value is the share read mod p, at a column it found
 *   wrong the share that party should hold.  It may as well be any other index below p - 1 (a party that lost its state, or one
 *   that joins under a new index); duplicates are allowed and the order of the targets only permutes the columns of values.
 *   r = 0 is plain interpolation through all columns, r = 1 detects only, and the order of the share columns changes no value.
 *   Every output is a function of the inputs alone and the three forms agree bit for bit, small-p rows included.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the corrected calls refuse; NULL targets or values;
 * num_targets = 0; a target >= p - 1; on the device num_targets >= 2^31, refused before the targets are read (the _host form has
 * no such bound: it reads every target it is given). */
/* the contract in plain C++ on the host cores: the Berlekamp-Welch routine of pvw_shamir_reconstruct_corrected_host, whose
 * quotient F_s is evaluated by Horner's rule at every target: what the kernels are tested against */
PVW_API int32_t pvw_shamir_evaluate_corrected_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                   const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                   size_t point_stride, const uint64_t* targets, size_t num_targets, uint64_t* values,
                                                   uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
/* device pointers (indices and targets stay HOST pointers, read before the call returns), asynchronous on `stream`.  The scratch is
 * the corrected call's block in the stream's workspace with the evaluation's regions behind it, sized by the call: under stream
 * capture the call needs an earlier call with the same (degree, count), at least as many targets and at least as many secrets on
 * that stream outside capture; without it: the error of pvw_shamir_reconstruct_corrected_device there, nothing enqueued.
 * Everything in the scratch that depends on the shares is cleared behind the call's last launch. */
PVW_API int32_t pvw_shamir_evaluate_corrected_device(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                     size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                     size_t point_stride, const uint64_t* targets, size_t num_targets,
                                                     uint64_t* d_values, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                     uint64_t* d_err_mask, void* stream);
/* host buffers (synchronous); the staged shares, secrets and values are cleared before the call returns.  Covered by the
 * concurrency promise above. */
PVW_API int32_t pvw_shamir_evaluate_corrected(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                              size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                              size_t point_stride, const uint64_t* targets, size_t num_targets, uint64_t* values,
                                              uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
/* Reconstruction with erasures: a share the caller KNOWS to be bad -- flagged by a checked decrypt, never arrived,
 * from a refused dealer -- costs one redundant column instead of two.  The arguments of the corrected and evaluate calls, and
 * directly behind point_stride: erased [num_secrets][W], W = ceil(count / 64), bit c % 64 of word c / 64 of row s set iff share
 * (s, c) is erased: the layout of err_mask, so one call's err_mask can be the next call's erased.  A device pointer in the
 * _device forms, a host pointer elsewhere; bits at columns >= count are ignored; NULL means no erasures, and every call is then
 * the corrected or evaluate call it extends, bit for bit on every output.
 *   For row s let eps_s be the number of erased columns, r = count - degree - 1 and E_s = (r - eps_s) / 2 (rounded down).
 *   Row s is DECODABLE iff eps_s <= r and some polynomial F_s of degree <= t disagrees with the row (read mod p) in at most E_s of
 *   the columns that are not erased in row s: the corrected call's definition on the sub-row of those columns.  F_s is then
 *   unique.  So 2 errors + erasures <= r per row; r erasures and no error still decode; eps_s > r is undecodable (a property of
 *   the row, not an argument error).
 *   decodable:   out[s] = F_s(0); nerr[s] = the number of non-erased columns that disagree; err_mask row s has exactly their
 *                bits (an erased column is never reported as an error); col_err[c] counts the decodable rows with an error at c;
 *                values[s][j] = F_s(targets[j] + 1): at an erased or wrong column the share that party should hold.
 *   undecodable: out = 0, nerr = PVW_SHAMIR_UNDECODABLE, mask row and values row 0, nothing added to col_err.
 *   The word stored at an erased position influences no output: it may be any 64-bit word.  Column order, target order, determinism and
 *   the agreement of the three forms (small p included) are those of the calls extended.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the extended call refuses, with its text; on the
 * device, for a call WITH a mask, also count - degree - 1 >= 4096 (the errata locator of a row has up to r + 1 coefficients; with
 * erased == NULL the bound is the one of the call extended, as everything else is; the corrected calls keep
 * their own bound).  Under stream capture: the rule of the extended device call, sized by a call WITH a mask (its scratch is the
 * larger: the public power matrices have r + 1 rows); the mask is read when the kernels run.  The host-buffer forms stage the mask
 * rows with the shares and are covered by the concurrency promise above. */
/* the contract in plain C++ on the host cores: per row the non-erased columns are compacted and decoded by the Berlekamp-Welch
 * routine of pvw_shamir_reconstruct_corrected_host with the same degree: what the kernels are tested against */
PVW_API int32_t pvw_shamir_reconstruct_erasures_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                     const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                     size_t point_stride, const uint64_t* erased, uint64_t* out, uint32_t* nerr,
                                                     uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_reconstruct_erasures_device(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                       size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                       size_t point_stride, const uint64_t* d_erased, uint64_t* d_out, uint32_t* d_nerr,
                                                       uint32_t* d_col_err, uint64_t* d_err_mask, void* stream);
PVW_API int32_t pvw_shamir_reconstruct_erasures(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                size_t point_stride, const uint64_t* erased, uint64_t* out, uint32_t* nerr,
                                                uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_erasures_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                  const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                  const uint64_t* erased, const uint64_t* targets, size_t num_targets, uint64_t* values,
                                                  uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_erasures_device(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                    size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                    size_t point_stride, const uint64_t* d_erased, const uint64_t* targets,
                                                    size_t num_targets, uint64_t* d_values, uint64_t* d_out, uint32_t* d_nerr,
                                                    uint32_t* d_col_err, uint64_t* d_err_mask, void* stream);
PVW_API int32_t pvw_shamir_evaluate_erasures(pvw_ctx* ctx, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                             size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                             size_t point_stride, const uint64_t* erased, const uint64_t* targets, size_t num_targets,
                                             uint64_t* values, uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
/* The mask from a decrypt report: bit (s, c) of mask_out [num_secrets][W] is set iff status[..] & status_bits is non-zero or
 * noise[..] > noise_bound, element (s, c) of status (u32) and noise (u64) at s * secret_stride + c * point_stride as the shares are.
 * Either array may be NULL, not both; both are only read (status is declared as the decrypt calls declare it, so their buffer
 * passes as it is).  Every word of mask_out is written, padding bits 0.  Strides (1, D) read the [party][dealer]
 * report of pvw_decrypt_all_*_checked / _plain in place (every dealer a secret), so decrypt-all -> mask -> decode stays on the
 * device.  PVW_ERR_INVALID_PARAMETERS, nothing written: NULL mask_out (or ctx), both arrays NULL, count or num_secrets 0, a
 * stride of 0; on the device count or num_secrets >= 2^31. */
PVW_API int32_t pvw_shamir_erasure_mask_host(uint32_t* status, const uint64_t* noise, uint32_t status_bits, uint64_t noise_bound,
                                             size_t count, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                             uint64_t* mask_out);
PVW_API int32_t pvw_shamir_erasure_mask_device(pvw_ctx* ctx, uint32_t* d_status, const uint64_t* d_noise, uint32_t status_bits,
                                               uint64_t noise_bound, size_t count, size_t num_secrets, size_t secret_stride,
                                               size_t point_stride, uint64_t* d_mask_out, void* stream);

/* ---- Packed Shamir shares: several secrets in one polynomial and one ciphertext ---------------------------
 * Franklin-Yung packing: `pack` = K >= 1 secrets per dealer sit at the points 0, -1, ..., -(K-1) of ONE polynomial, so S secrets
 * take S / K ciphertexts, encrypts, decrypts and wire bytes, for K - 1 of threshold slack.  The reference has no sharing code:
 * the contract is the library's own.  All arithmetic in Z_p, p = plain_modulus; degree = t >= 0 random coefficients:
 *   f_d(x) = sum_{j<K} s_{d,j} L_j(x)  +  Z(x) (a_{d,1} + a_{d,2} x + ... + a_{d,t} x^(t-1))
 *   L_j = the Lagrange basis polynomial of the point -j among 0, -1, ..., -(K-1);  Z(x) = x (x+1) ... (x+K-1)
 *   shares[d][i] = f_d(i + 1) for the global party index i
 * deg f_d <= t + K - 1; f_d(-j) = s_{d,j}; any t + K shares determine all K secrets, and with t >= 1 any t shares are
 * independent of them.  a_{d,j} (j = 1..t) are exactly the draws of 8.9 (same key, stream id and rule); coeffs [D][t] replaces
 * the draw.  secrets [D][K] are dealer-major, any word read mod p.  With K = 1 the polynomial is s_d + a_{d,1} x + ... + a_{d,t} x^t:
 * every packed call with pack = 1 is bit-equal to the 8.9 call it extends.
 * PVW_ERR_INVALID_PARAMETERS before any device work (after the checks of the pvw_encrypt_multi* call a deal extends): pack = 0,
 * degree + pack > n, p composite or >= 2^62, p < n + pack (the points 1..n and p-K+1..p-1, 0 must be distinct; p > n when
 * K = 1), num_dealers = 0, NULL arguments by the rules of 8.9 (seeds may be NULL iff coeffs is given or degree = 0).
 * The way back: pvw_shamir_reconstruct_packed on the host, or pvw_shamir_evaluate_corrected* with polynomial degree t + K - 1:
 * `out` is secret 0 and the target index p - 1 - j (the point -j) gives secret j. */
/* the contract in plain C++ on the host cores (no GPU needed), all n columns: what the kernels are tested against */
PVW_API int32_t pvw_shamir_shares_packed_host(const pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack,
                                              uint32_t degree, uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs,
                                              uint64_t* shares_out);
/* device pointers (seeds stays a HOST pointer), asynchronous on `stream`.  The public weights L_j(i + 1) and Z(i + 1) / (i + 1) are
 * made on the device into the stream's workspace, sized by the call: under stream capture a call needs an earlier call on that
 * stream outside capture with at least as many pack x columns words, otherwise PVW_ERR_INVALID_PARAMETERS and nothing enqueued.
 * A captured call holds the address of that block: a later packed call on the same stream, outside capture, that needs MORE words
 * replaces the block, and graphs captured before it must be captured again (as for the blocks of the checked and corrected
 * reconstruction).  Size the stream for the largest pack first.
 * Columns of a sharded context as 8.9. */
PVW_API int32_t pvw_shamir_shares_packed_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack,
                                                uint32_t degree, uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs,
                                                uint64_t* d_shares, void* stream);
/* host buffers (synchronous), staged in bounded pieces; the staged secrets, coefficients and shares are cleared before the call
 * returns */
PVW_API int32_t pvw_shamir_shares_packed(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                         uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out);
/* Deal: pvw_deal_shares_packed*(secrets [D][pack], D, pack, degree, p, seeds, ...) == pvw_encrypt_multi*(shares, D, n, seeds, ...)
 * bit for bit with shares = pvw_shamir_shares_packed_host(secrets, D, pack, degree, p, seeds, NULL): both representations, both
 * sides of the dealer-count dispatch, sharded contexts.  Everything else as pvw_deal_shares*: the _rs forms leave c + D in the
 * state, pvw_prepare(PVW_PREPARE_MFMA) covers the share scratch, and under stream capture the weights must have been sized as
 * for pvw_shamir_shares_packed_device (the error of pvw_encrypt_multi_device otherwise, nothing enqueued). */
PVW_API int32_t pvw_deal_shares_packed(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                       uint64_t plain_modulus, const uint8_t* seeds /*[D][32]*/, uint64_t* c1_out, uint64_t* c2_out,
                                       uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_packed_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack,
                                              uint32_t degree, uint64_t plain_modulus, const uint8_t* seeds, uint64_t* d_c1,
                                              uint64_t* d_c2, uint32_t out_repr, void* stream);
PVW_API int32_t pvw_deal_shares_packed_rs(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                          uint64_t plain_modulus, void* st, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_packed_rs_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack,
                                                 uint32_t degree, uint64_t plain_modulus, void* st, uint64_t* d_c1, uint64_t* d_c2,
                                                 uint32_t out_repr, void* stream);
/* Reconstruction, host only (no GPU, no context), like pvw_shamir_reconstruct: out[r][j] = F_r(-j), j < pack, from the Lagrange
 * weights of the points indices[i] + 1 at each of 0, -1, ..., -(pack-1), computed once.  shares [num_rows][count], out
 * [num_rows][pack].  The rules of pvw_shamir_reconstruct, plus pack >= 1 and every index < p - pack.  count must be at least
 * degree + pack for the result to be the secrets; the routine cannot know the degree and does not check. */
PVW_API int32_t pvw_shamir_reconstruct_packed(uint64_t plain_modulus, uint32_t pack, const uint64_t* indices, const uint64_t* shares,
                                              size_t count, size_t num_rows, uint64_t* out);

/* ---- Shamir shares over a prime field of up to 256 bits: wide shares as limb ciphertexts -------------------
 * The family above works in Z_p with p < 2^62; a PVSS / DKG round most often shares a scalar of an elliptic-curve group
 * (secp256k1's order, BLS12-381's r, the Ed25519 group order, 2^255 - 19).  This family is the same dealing end over such a
 * field.  The reference has no sharing code: the contract is the library's own.  No call above changes; p >= 2^62 stays
 * refused by every one of them.
 *   A wide element is PVW_WIDE_WORDS = 4 little-endian uint64_t words.  plain_modulus (a HOST pointer in every form) is such an
 *   element: an odd prime with n < p < 2^256.  Primality is checked on the host, before any device work, by Miller-Rabin over
 *   the 32 prime bases 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101,
 *   103, 107, 109, 113, 127, 131 (a single-word p by the deterministic test of the family above).  A composite or even p,
 *   p <= n, degree >= n, num_dealers = 0 or a NULL argument: PVW_ERR_INVALID_PARAMETERS.
 *   f_d(x) = s_d + a_{d,1} x + ... + a_{d,t} x^t mod p and shares[d][i] = f_d(i + 1), i the global party index.  secrets [D][4]
 *   and explicit coefficients [D][t][4] are wide words that mean w mod p: any word is accepted, 2^256 - 1 included.  t = 0
 *   copies the secret and draws nothing.
 *   a_{d,j} = the first accepted attempt of the ChaCha8 stream (PVW_DOM_SHAMIR << 32) | j under dealer d's key: an attempt is
 *   four consecutive next_u64() words, word 0 least significant, masked to the low bitlen(p) bits and accepted when below p
 *   (at least every second attempt).  For p < 2^62 these are NOT the coefficients pvw_shamir_shares* draws.
 *   Limbs: a share is cut into NL = ceil(bitlen(p) / limb_bits) limbs of limb_bits bits, 16 <= limb_bits <= 62 and
 *   NL <= PVW_WIDE_MAX_LIMBS = 16, limb w = (share >> (w limb_bits)) mod 2^limb_bits.  Each limb is one PVW plaintext (below
 *   2^63, encryption.rs:195); ciphertext v = d NL + w carries limb w of dealer d's shares.  With limb_bits = 52 (5 limbs at 256
 *   bits) the limb-wise sum of up to 2048 dealers stays below 2^63, so pvw_ct_sum* / pvw_decrypt_*sum* aggregate a wide
 *   sharing unchanged, limb by limb, and pvw_shamir_wide_from_limbs_host folds the summed limbs back mod p.
 *   Keys: the shares-alone calls take seeds [D][32], dealer d's coefficient key.  The deal calls take seeds [D NL][32]: vector v
 *   is encrypted exactly as vector v of pvw_encrypt_multi, and dealer d's coefficients are drawn under the key of vector d NL;
 *   a dealer never shares one r between two of its limbs.  _rs forms: vector v's key is call_seed(S, c + v), and the state
 *   ends at c + D NL. */
#define PVW_WIDE_WORDS 4
#define PVW_WIDE_MAX_LIMBS 16
/* NL for (p, limb_bits); host only, no context.  p even or below 3, limb_bits outside [16, 62], NL > 16: INVALID_PARAMETERS */
PVW_API int32_t pvw_shamir_wide_limbs(const uint64_t* plain_modulus, uint32_t limb_bits, uint32_t* num_limbs);
/* shares [D][n][4].  The host routine (no GPU needed; what the kernel is tested against) writes every column; the device
 * routines write columns [party_lo, party_hi) of a sharded context and leave the others untouched.  The _device form takes
 * device pointers (seeds and plain_modulus stay HOST pointers), is asynchronous on `stream`, allocates nothing and may be
 * captured.  The host-buffer form stages the dealers in bounded pieces and clears what it staged before it returns. */
PVW_API int32_t pvw_shamir_shares_wide_host(const pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                            const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs,
                                            uint64_t* shares_out);
PVW_API int32_t pvw_shamir_shares_wide_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                              const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs,
                                              uint64_t* d_shares, void* stream);
PVW_API int32_t pvw_shamir_shares_wide(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                       const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs,
                                       uint64_t* shares_out);
/* Deal: pvw_encrypt_multi* on D NL vectors, outputs c1 [D NL]..., c2 [D NL]..., bit for bit what pvw_encrypt_multi* gives for
 * the limb planes (pvw_shamir_wide_to_limbs_host per dealer) of pvw_shamir_shares_wide_host(..., seeds[d NL], NULL): both
 * representations, both sides of the dealer-count dispatch (by D NL), sharded contexts.  The checks of pvw_encrypt_multi* come
 * first, then the ones above.  Capture rules and the wipe of the share scratch as pvw_deal_shares*: after
 * pvw_prepare(PVW_PREPARE_MFMA) the _device forms neither allocate nor synchronise and may be captured, and every replay of the
 * _rs form deals a fresh sharing. */
PVW_API int32_t pvw_deal_shares_wide(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                     const uint64_t* plain_modulus, uint32_t limb_bits, const uint8_t* seeds, uint64_t* c1_out,
                                     uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_wide_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                            const uint64_t* plain_modulus, uint32_t limb_bits, const uint8_t* seeds, uint64_t* d_c1,
                                            uint64_t* d_c2, uint32_t out_repr, void* stream);
PVW_API int32_t pvw_deal_shares_wide_rs(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                        const uint64_t* plain_modulus, uint32_t limb_bits, void* st, uint64_t* c1_out,
                                        uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_wide_rs_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                               const uint64_t* plain_modulus, uint32_t limb_bits, void* st, uint64_t* d_c1,
                                               uint64_t* d_c2, uint32_t out_repr, void* stream);
/* Host only: values [count][4] -> limbs_out [num_limbs][count] (a value that does not fit num_limbs limbs: INVALID_PARAMETERS),
 * and back: out[i] = sum_w limbs[w][i] 2^(w limb_bits) mod p, where each input word is ANY uint64_t -- a limb, or a sum of limbs. */
PVW_API int32_t pvw_shamir_wide_to_limbs_host(const uint64_t* values, size_t count, uint32_t limb_bits, uint32_t num_limbs,
                                              uint64_t* limbs_out);
PVW_API int32_t pvw_shamir_wide_from_limbs_host(const uint64_t* plain_modulus, const uint64_t* limbs, size_t count, uint32_t limb_bits,
                                                uint32_t num_limbs, uint64_t* out);
/* Reconstruction, host only: Lagrange at 0 of the points indices[i] + 1.  shares [num_secrets][count][4] (any words, read mod
 * p), out [num_secrets][4].  The rules of pvw_shamir_reconstruct: count = 0, a duplicate index, an index >= p - 1, a composite
 * p: INVALID_PARAMETERS; count must be at least degree + 1 for the result to be the secret. */
PVW_API int32_t pvw_shamir_reconstruct_wide(const uint64_t* plain_modulus, const uint64_t* indices, const uint64_t* shares, size_t count,
                                            size_t num_secrets, uint64_t* out);
/* SELF-TEST: the kernel's own Horner step on the device, out[i] = (acc[i] x[i] + add[i]) mod p for acc, add [count][4] below
 * p and x [count] below 2^32 (anything else: INVALID_PARAMETERS).  It exists because x near 2^32 cannot be reached through n. */
PVW_API int32_t pvw_selftest_shamir_wide_step(pvw_ctx* ctx, const uint64_t* plain_modulus, const uint64_t* acc, const uint64_t* x,
                                              const uint64_t* add, size_t count, uint64_t* out);

/* ---- Packed Shamir shares over a prime field of up to 256 bits: the polynomial of 8.14 with the elements, draws
 * and limbs of 8.18.  `pack` = K >= 1 secrets per dealer, `degree` = t >= 0 random coefficients, all arithmetic in Z_p:
 *   f_d(x) = sum_{j<K} s_{d,j} L_j(x)  +  Z(x) (a_{d,1} + a_{d,2} x + ... + a_{d,t} x^(t-1))  mod p
 *   L_j = the Lagrange basis polynomial of the point -j among 0, -1, ..., -(K-1);  Z(x) = x (x+1) ... (x+K-1)
 *   shares[d][i] = f_d(i + 1), i the global party index; a share is four words, fully reduced
 * secrets [D][K][4] are dealer-major and coeffs [D][t][4] optional; any words are accepted and read mod p.  a_{d,j} (j = 1..t) are
 * exactly the draws of 8.18; degree = 0 draws nothing and needs no seeds.  With K = 1 the polynomial is that of 8.18 (L_0 = 1,
 * Z = x): every call below with pack = 1 is bit-equal to the wide call it extends, for shares and for ciphertexts.  Limbs, keys
 * and the _rs counter as pvw_deal_shares_wide*: seeds [D NL][32], dealer d's coefficients drawn under the key of vector d NL, the
 * state ends at c + D NL; the shares-alone calls take seeds [D][32].  S wide secrets cost S NL / K ciphertexts.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the call being extended refuses, then pack = 0,
 * pack > PVW_WIDE_MAX_PACK (the weights are 32 pack columns bytes: 128 MiB at 4096 columns), degree + pack > n,
 * n + pack - 1 >= 2^32 (the weights are built with 32-bit multipliers), p < n + pack (as wide integers; p <= n when K = 1).
 * The weights L_j(i + 1) and Z(i + 1) are public and made on the device into a block of the stream's workspace, sized by the
 * call: under stream capture the _device forms need an earlier call of this kind on that stream outside capture with at least as
 * many pack x columns words (and pvw_prepare(PVW_PREPARE_MFMA) for the deals), otherwise the error of pvw_encrypt_multi_device
 * and nothing enqueued.  A later call that needs more words replaces the block: capture again, as for 8.14.
 * The way back: pvw_ct_sum*, pvw_decrypt_*sum*, pvw_shamir_wide_from_limbs_* and the wide reconstruct / evaluate calls take a
 * packed sharing as a polynomial of degree t + K - 1; pvw_shamir_reconstruct_packed_wide reads the K secrets off its shares. */
#define PVW_WIDE_MAX_PACK 1024
/* the contract on the host cores (no GPU needed), all n columns: what the kernels are tested against.  shares [D][n][4] */
PVW_API int32_t pvw_shamir_shares_packed_wide_host(const pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack,
                                                   uint32_t degree, const uint64_t* plain_modulus, const uint8_t* seeds,
                                                   const uint64_t* coeffs, uint64_t* shares_out);
PVW_API int32_t pvw_shamir_shares_packed_wide_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack,
                                                     uint32_t degree, const uint64_t* plain_modulus, const uint8_t* seeds,
                                                     const uint64_t* d_coeffs, uint64_t* d_shares, void* stream);
PVW_API int32_t pvw_shamir_shares_packed_wide(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                              const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs,
                                              uint64_t* shares_out);
/* Deal: pvw_encrypt_multi* on D NL vectors, bit for bit what it gives for the limb planes of
 * pvw_shamir_shares_packed_wide_host(..., seeds[d NL], NULL): both representations, both sides of the dealer-count dispatch (by
 * D NL), sharded contexts.  Every replay of a captured _rs form deals a fresh sharing. */
PVW_API int32_t pvw_deal_shares_packed_wide(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                            const uint64_t* plain_modulus, uint32_t limb_bits, const uint8_t* seeds, uint64_t* c1_out,
                                            uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_packed_wide_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack,
                                                   uint32_t degree, const uint64_t* plain_modulus, uint32_t limb_bits,
                                                   const uint8_t* seeds, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream);
PVW_API int32_t pvw_deal_shares_packed_wide_rs(pvw_ctx* ctx, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                               const uint64_t* plain_modulus, uint32_t limb_bits, void* st, uint64_t* c1_out,
                                               uint64_t* c2_out, uint32_t out_repr);
PVW_API int32_t pvw_deal_shares_packed_wide_rs_device(pvw_ctx* ctx, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack,
                                                      uint32_t degree, const uint64_t* plain_modulus, uint32_t limb_bits, void* st,
                                                      uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream);
/* Reconstruction, host only (no GPU, no context): out[r][j] = F_r(-j), j < pack, from the Lagrange weights of the points
 * indices[i] + 1 at each of 0, -1, ..., -(pack-1), computed once, then pack dot products per row.  shares [num_rows][count][4]
 * (any words, read mod p), out [num_rows][pack][4].  The rules of pvw_shamir_reconstruct_wide, plus pack >= 1 and every index
 * < p - pack.  count must be at least degree + pack for the result to be the secrets. */
PVW_API int32_t pvw_shamir_reconstruct_packed_wide(const uint64_t* plain_modulus, uint32_t pack, const uint64_t* indices,
                                                   const uint64_t* shares, size_t count, size_t num_rows, uint64_t* out);

/* ---- The receiving end over a prime field of up to 256 bits: the fold of decrypted limbs on the device, and
 * checked reconstruction with wide elements.  The contract is the library's own.  plain_modulus is a HOST pointer to an odd
 * prime below 2^256 in every form, checked as above.
 * Fold: out[i] = sum_w limbs[w * limb_stride + i * elem_stride] 2^(w limb_bits) mod p for i < count, out [count][4]; each input
 *   word is ANY uint64_t, a limb or a sum of limbs.  Strides (count, 1) read the planes of pvw_shamir_wide_from_limbs_host;
 *   strides (1, NL) read the [party][dealer NL + w] result of pvw_decrypt_all* in place, as P D elements in [party][dealer]
 *   order.  Device pointers, asynchronous on `stream`, allocates nothing, may be captured; bit-equal to the host form.
 *   PVW_ERR_INVALID_PARAMETERS before any device work: what pvw_shamir_wide_from_limbs_host refuses, a NULL ctx, a stride of 0. */
PVW_API int32_t pvw_shamir_wide_from_limbs_device(pvw_ctx* ctx, const uint64_t* plain_modulus, const uint64_t* d_limbs, size_t count,
                                                  size_t limb_stride, size_t elem_stride, uint32_t limb_bits, uint32_t num_limbs,
                                                  uint64_t* d_out, void* stream);
/* Checked reconstruction: the contract of pvw_shamir_reconstruct_checked*  word for word, with wide elements.
 *   degree = t.  indices [count]: distinct global party indices, a HOST pointer in every form; the points are the INTEGERS
 *   x_c = indices[c] + 1, each below p (an index of 2^64 - 1 is legal when p > 2^64 + 1).  shares: num_secrets rows, element
 *   (s, c) is the four words at shares + 4 (s * secret_stride + c * point_stride) (strides in elements; any words, read mod p):
 *   strides (count, 1) read [secret][party][4], strides (1, D) the fold's [party][dealer][4] output in place, every dealer a
 *   secret.  Basis: columns 0..t in the caller's order; extras: columns t+1..count-1.  F_s: the polynomial of degree <= t
 *   through the basis points of secret s.
 *   out [num_secrets][4] = F_s(0).  bad [num_secrets] (or NULL): how many extras c have share(s, c) mod p != F_s(x_c).
 *   col_bad [count] (or NULL): for each column, how many secrets deviate there; 0 for the basis columns.
 *   One wrong extra share is flagged at exactly that (s, c) and out is right; one wrong basis share of secret s makes out[s]
 *   wrong and flags EVERY extra of s.  The routine detects; it neither corrects errors nor searches for a basis.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: NULL plain_modulus / indices / shares / out (or ctx),
 * num_secrets = 0, count < degree + 1, duplicate indices, an index whose point is not below p, a composite or even p, a stride
 * of 0 (and, on the device, count or num_secrets >= 2^31). */
/* the contract in plain C++ on the host cores (no context, no GPU): what the kernels are tested against */
PVW_API int32_t pvw_shamir_reconstruct_wide_checked_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                         size_t count, const uint64_t* shares, size_t num_secrets,
                                                         size_t secret_stride, size_t point_stride, uint64_t* out, uint32_t* bad,
                                                         uint32_t* col_bad);
/* device pointers (indices and plain_modulus stay HOST pointers, read before the call returns), asynchronous on `stream`.  The
 * wide weight matrix [t+1][count-t][4] lives in the stream's workspace, sized by the call (134 MB at count 4096, t 2047): under
 * stream capture the call needs an earlier call with the same (degree, count) on that stream outside capture; without it: the
 * error of pvw_shamir_reconstruct_checked_device, nothing enqueued. */
PVW_API int32_t pvw_shamir_reconstruct_wide_checked_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                           const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                           size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                           uint64_t* d_out, uint32_t* d_bad, uint32_t* d_col_bad, void* stream);
/* host buffers (synchronous), staged in bounded pieces; the staged shares and secrets are cleared before the call returns */
PVW_API int32_t pvw_shamir_reconstruct_wide_checked(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                    const uint64_t* indices, size_t count, const uint64_t* shares, size_t num_secrets,
                                                    size_t secret_stride, size_t point_stride, uint64_t* out, uint32_t* bad,
                                                    uint32_t* col_bad);
/* Corrected reconstruction over a prime field of up to 256 bits: the contract of
 * pvw_shamir_reconstruct_corrected*  word for word, with wide elements.  Arguments as for
 * pvw_shamir_reconstruct_wide_checked*.  No column is a basis: with r = count - degree - 1 redundant columns, row s is DECODABLE
 * iff some polynomial F_s of degree <= t disagrees with it in at most E = r / 2 columns (F_s is then unique), whichever columns.
 *   out [num_secrets][4] = F_s(0), 0 for an undecodable row.  nerr [num_secrets] (or NULL): the number of disagreeing columns, or
 *   PVW_SHAMIR_UNDECODABLE.  col_err [count] (or NULL): for each column, in how many decodable rows it disagrees.  err_mask
 *   [num_secrets][ceil(count / 64)] (or NULL): bit c % 64 of word c / 64 of row s set iff column c disagrees in row s; a zero
 *   row for an undecodable secret, padding bits 0.
 *   r = 0 is plain interpolation through all columns, r = 1 detects only.  The order of the columns changes no output; mask
 *   bits and col_err move with their columns.  The three forms agree bit for bit on every input.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what pvw_shamir_reconstruct_wide_checked* refuses, in its
 * order; and, in the two device forms, r / 2 + 1 > PVW_SHAMIR_WIDE_MAX_LOCATOR (r >= 4096): the two polynomials of one wave
 * take 2 (E + 1) 32 bytes of LDS, 128 KiB at the bound. */
#define PVW_SHAMIR_WIDE_MAX_LOCATOR 2048
/* the contract in plain C++ on the host cores (no context, no GPU), Berlekamp-Welch: cubic in count, a reference */
PVW_API int32_t pvw_shamir_reconstruct_wide_corrected_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                           size_t count, const uint64_t* shares, size_t num_secrets,
                                                           size_t secret_stride, size_t point_stride, uint64_t* out, uint32_t* nerr,
                                                           uint32_t* col_err, uint64_t* err_mask);
/* device pointers (indices and plain_modulus stay HOST pointers, read before the call returns), asynchronous on `stream`.  The
 * public matrices and the per-secret scratch live in the stream's workspace, sized by the call: under stream capture the call
 * needs an earlier call with the same (degree, count) and at least as many secrets on that stream outside capture; without it:
 * the error of pvw_shamir_reconstruct_wide_checked_device, nothing enqueued. */
PVW_API int32_t pvw_shamir_reconstruct_wide_corrected_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                             const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                             size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                             uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                             uint64_t* d_err_mask, void* stream);
/* host buffers (synchronous), staged in bounded pieces; the staged shares and secrets are cleared before the call returns */
PVW_API int32_t pvw_shamir_reconstruct_wide_corrected(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                      const uint64_t* indices, size_t count, const uint64_t* shares,
                                                      size_t num_secrets, size_t secret_stride, size_t point_stride, uint64_t* out,
                                                      uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
/* Reconstruction with erasures over a prime field of up to 256 bits: the contract of
 * pvw_shamir_reconstruct_erasures*  with wide elements.  A wide share arrives as num_limbs ciphertexts and is lost
 * as soon as ONE of them is flagged by the checked decrypt, never arrived or came from a refused dealer; the combiner knows that
 * before it reconstructs, and a share it KNOWS to be bad costs one redundant column instead of two.  The arguments of the
 * matching pvw_shamir_reconstruct_wide_corrected* form in its order, and directly behind point_stride:
 * erased [num_secrets][W], W = ceil(count / 64), bit c % 64 of word c / 64 of row s set iff share (s, c) is erased: the layout of
 * err_mask, so one call's err_mask can be the next call's erased.  A device pointer in the _device form, a host pointer
 * elsewhere; bits at columns >= count are ignored; NULL means no erasures, and the call is then the wide corrected call, bit for
 * bit on every output: behind the argument checks it IS that call.
 *   For row s let eps_s be the number of erased columns, r = count - degree - 1 and E_s = (r - eps_s) / 2 (rounded down).
 *   Row s is DECODABLE iff eps_s <= r and some polynomial F_s of degree <= t disagrees with the row (read mod p) in at most E_s of
 *   the columns that are not erased in row s: the wide corrected call's definition on the sub-row of those columns.  F_s is then
 *   unique.  So 2 errors + erasures <= r per row; r erasures and no error still decode; eps_s > r is undecodable (a property of
 *   the row, not an argument error).
 *   decodable:   out[s][4] = F_s(0); nerr[s] = the number of non-erased columns that disagree; err_mask row s has exactly their
 *                bits (an erased column is never reported as an error); col_err[c] counts the decodable rows with an error at c.
 *   undecodable: out = 0, nerr = PVW_SHAMIR_UNDECODABLE, a zero mask row, nothing added to col_err.
 *   The four words stored at an erased position influence no output: they may be anything, 2^256 - 1 included.  Column order,
 *   determinism and the agreement of the three forms on every input (small p included) are those of the call extended.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the wide corrected forms refuse, with their texts and
 * in their order.  The device forms keep exactly that call's bound, with or without a mask: r >= 4096 is refused.  No further
 * refusal is needed: with a mask one wave keeps the erasure locator Gamma [eps + 1] and the two polynomials C, B [E_s + 1] of the
 * recurrence in LDS, eps + 1 + 2 ((r - eps) / 2 + 1) <= r + 3 elements of 32 bytes, 131 136 bytes at r = 4095, and one gfx950
 * workgroup may take 160 KiB.  No new status code.
 * Under stream capture: the rule of the wide corrected device call, sized by a call WITH a mask (its scratch is the larger: the
 * locators and the public power matrix have r + 1 rows); a stream sized by maskless calls alone is refused with this call's own
 * error and nothing is enqueued.  The mask is read when the kernels run, so a replay may see a new mask.  The host-buffer form
 * stages the mask rows of a piece with its shares and is covered by the concurrency promise above.  The mask, the erasure
 * locators and the Forney syndromes are not secret; the secret regions are those of the call extended. */
/* the contract in plain C++ on the host cores: per row the non-erased columns are compacted and decoded by the Berlekamp-Welch
 * routine of pvw_shamir_reconstruct_wide_corrected_host with the same degree, mask bits and col_err scattered back: what the
 * kernels are tested against, sharing nothing with them */
PVW_API int32_t pvw_shamir_reconstruct_wide_erasures_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                          size_t count, const uint64_t* shares, size_t num_secrets,
                                                          size_t secret_stride, size_t point_stride, const uint64_t* erased,
                                                          uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_reconstruct_wide_erasures_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                            const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                            size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                            const uint64_t* d_erased, uint64_t* d_out, uint32_t* d_nerr,
                                                            uint32_t* d_col_err, uint64_t* d_err_mask, void* stream);
PVW_API int32_t pvw_shamir_reconstruct_wide_erasures(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                     const uint64_t* indices, size_t count, const uint64_t* shares,
                                                     size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                     const uint64_t* erased, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                                     uint64_t* err_mask);
/* Share repair over a prime field of up to 256 bits: the contract of pvw_shamir_evaluate_corrected* (8.13) and
 * pvw_shamir_evaluate_erasures* (8.16) with wide elements.  The arguments of the matching pvw_shamir_reconstruct_wide_corrected* /
 * _wide_erasures* form in its order (erased directly behind point_stride), then targets, num_targets and values, then the four
 * outputs out, nerr, col_err, err_mask, and stream in the _device form.
 *   targets [num_targets]: a HOST array of global party indices in every form, like indices; the point of target j is the integer
 *   targets[j] + 1, which must be below p (a target of 2^64 - 1 is legal when p > 2^64 + 1, as for indices).
 *   values [num_secrets][num_targets][4], dense and row-major, may not be NULL; out may be NULL here.
 *   Decodability, F_s, out, nerr, col_err and err_mask are those of the wide corrected call without a mask and of the wide
 *   erasures call with one, bit for bit: one decode yields every report.
 *   decodable row:   values[s][j] = F_s(targets[j] + 1) mod p, fully reduced, four words.
 *   undecodable row: its row of values is 0 (eps_s > r, too many errors, a root of the error locator on an erased point).
 *   A target may be one of the indices: at a column the decode found right the value is the share read mod p, at a wrong or an
 *   erased column the share that party should hold.  The words at an erased position influence nothing, 2^256 - 1 included.
 *   Duplicates are allowed; the order of the targets only permutes the columns of values; the order of the share columns changes
 *   no value; r = 0 is plain interpolation through all columns.  The three forms agree bit for bit on every input, small-p rows
 *   that decode to a polynomial nobody dealt included.  erased == NULL is the wide evaluate-corrected call bit for bit: behind
 *   the argument checks it IS that call.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the matching wide corrected / erasures form refuses,
 * with its texts and in its order (the device forms' bound included, unchanged: r >= 4096 is refused); then NULL targets or
 * values, num_targets = 0, a target whose point is not below p; on the device num_targets >= 2^31, checked before the targets
 * are walked.  No new status code and no new LDS bound: the evaluation needs no LDS beyond the tile product's.
 * Under stream capture: an earlier call of this kind on that stream outside capture with the same (degree, count), at least as
 * many targets and at least as many secrets, and with a mask if this one has a mask; otherwise the call fails with its own error
 * and enqueues nothing.  The host-buffer forms stage through the wide corrected call's staging (the mask rows of a piece with its
 * shares), are synchronous and are covered by the concurrency promise above.  Cleared behind the last launch: M, y o M, the
 * unscaled sums and the stand-in for out, and in the host-buffer form the staged shares, out and values; the public matrices, the
 * syndromes, the locators and their values at the public targets are not secret. */
/* the contract in plain C++ on the host cores: the Berlekamp-Welch routine of pvw_shamir_reconstruct_wide_corrected_host (on the
 * compacted sub-row with a mask) holds F_s as coefficients and evaluates them by Horner's rule at every target */
PVW_API int32_t pvw_shamir_evaluate_wide_corrected_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                        size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                        size_t point_stride, const uint64_t* targets, size_t num_targets,
                                                        uint64_t* values, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                                        uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_wide_corrected_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                          const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                          size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                          const uint64_t* targets, size_t num_targets, uint64_t* d_values,
                                                          uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask,
                                                          void* stream);
PVW_API int32_t pvw_shamir_evaluate_wide_corrected(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                   size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                   size_t point_stride, const uint64_t* targets, size_t num_targets, uint64_t* values,
                                                   uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_wide_erasures_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                       size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                       size_t point_stride, const uint64_t* erased, const uint64_t* targets,
                                                       size_t num_targets, uint64_t* values, uint64_t* out, uint32_t* nerr,
                                                       uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_wide_erasures_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                         const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                         size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                         const uint64_t* d_erased, const uint64_t* targets, size_t num_targets,
                                                         uint64_t* d_values, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                         uint64_t* d_err_mask, void* stream);
PVW_API int32_t pvw_shamir_evaluate_wide_erasures(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                  size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                                  size_t point_stride, const uint64_t* erased, const uint64_t* targets,
                                                  size_t num_targets, uint64_t* values, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                                  uint64_t* err_mask);
/* The mask of wide shares from a per-limb decrypt report: the arguments of pvw_shamir_erasure_mask_* plus num_limbs and
 * limb_stride.  Bit (s, c) of mask_out [num_secrets][W] is set iff, for some w < num_limbs, the element at
 * s * secret_stride + c * point_stride + w * limb_stride has status & status_bits non-zero or noise > noise_bound.  Either array
 * may be NULL, not both; both are only read (status is declared as the decrypt calls declare it, so their buffer passes as it
 * is).  Every word of mask_out is written, padding bits 0.  Strides (NL, D NL, 1) with NL = num_limbs read the
 * [party][dealer NL + w] report of pvw_decrypt_all_*_checked / _plain in place (every dealer a secret), so decrypt-all -> mask ->
 * fold -> decode stays on the device.  With num_limbs = 1 the call is pvw_shamir_erasure_mask_*, bit for bit.
 * PVW_ERR_INVALID_PARAMETERS, nothing written: what pvw_shamir_erasure_mask_* refuses, in its order, then num_limbs = 0 and
 * limb_stride = 0. */
PVW_API int32_t pvw_shamir_wide_erasure_mask_host(uint32_t* status, const uint64_t* noise, uint32_t status_bits, uint64_t noise_bound,
                                                  size_t count, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                  uint32_t num_limbs, size_t limb_stride, uint64_t* mask_out);
PVW_API int32_t pvw_shamir_wide_erasure_mask_device(pvw_ctx* ctx, uint32_t* d_status, const uint64_t* d_noise, uint32_t status_bits,
                                                    uint64_t noise_bound, size_t count, size_t num_secrets, size_t secret_stride,
                                                    size_t point_stride, uint32_t num_limbs, size_t limb_stride,
                                                    uint64_t* d_mask_out, void* stream);
/* SELF-TEST: the kernels' general product on the device, out[i] = a[i] b[i] mod p for a, b [count][4] below p (anything else:
 * INVALID_PARAMETERS). */
PVW_API int32_t pvw_selftest_shamir_wide_mul(pvw_ctx* ctx, const uint64_t* plain_modulus, const uint64_t* a, const uint64_t* b,
                                             size_t count, uint64_t* out);

/* decode_scalar_pvw_rns alone, on the device: noisy [D][L][l] power basis (host) -> out_u64 [D] */
PVW_API int32_t pvw_decode(pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64);
/* the same with host big integers on the host cores (no GPU needed): an independent
 * implementation kept as a cross-check of the device algorithm and for GPU-less tooling */
PVW_API int32_t pvw_decode_host(const pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64);
/* device pointers: d_noisy -> d_out [D].  pvw_decrypt_batch uses this, so only D x u64 leave the GPU. */
PVW_API int32_t pvw_decode_device(pvw_ctx* ctx, const uint64_t* d_noisy, size_t count, uint64_t* d_out,
                                  void* stream);
/* SELF-TEST hook: runs the device decode algorithm (pvw_decode.h) on the host so it can be checked
 * without a GPU.  No product path calls it. */
PVW_API int32_t pvw_selftest_decode_fixed(const pvw_ctx* ctx, const uint64_t* noisy, size_t count,
                                          uint64_t* out_u64);

/* SELF-TEST: C[32][32] (int32) = A[32][32] * B[32][32] (int8, row-major) with one i8 MFMA fetched
 * through the lane maps the digit-GEMM kernels assume. */
PVW_API int32_t pvw_selftest_mfma_i8(pvw_ctx* ctx, const int8_t* a, const int8_t* b, int32_t* out);
/* SELF-TEST: key hygiene.  SecretKey is Zeroize + ZeroizeOnDrop in the reference (src/keys/secret_key.rs:20-30);
 * here every device region that held key material during pvw_keygen / pvw_decrypt_* / pvw_sample_secret_keys
 * (uploaded coefficients, NTT(sk), key errors, their tiled / digitised copies) is cleared on the call's stream
 * before the call returns its workspace.  Reports how many 64-bit words of those regions (as declared by the
 * last such call on each pooled workspace) are not zero, and how many were scanned. */
PVW_API int32_t pvw_selftest_secret_residue(pvw_ctx* ctx, uint64_t* nonzero_words, uint64_t* scanned_words);
/* SELF-TEST: SipHash-c-d of msg under (k0, k1) -- the hash behind pvw_crs_seed_from_tag, exposed so that it can be
 * pinned against the published SipHash-2-4 vector */
PVW_API int32_t pvw_selftest_siphash(const uint8_t* msg, size_t len, uint64_t k0, uint64_t k1, int32_t c_rounds,
                                     int32_t d_rounds, uint64_t* out);
/* SELF-TEST (host only, no GPU): the short path of the device gadget decode (decode_scalar_pvw_rns,
 * src/crypto/decryption.rs:10-247) restated sequentially with the same arithmetic -- candidates confirmed on every limb,
 * noise_{l-1} proven from the residues, the chain to a fixed point.  short_path[d] (may be NULL) = 1 where every proof
 * held; elsewhere the value comes from pvw_selftest_decode_fixed's algorithm.  No product path calls it. */
PVW_API int32_t pvw_selftest_decode_shortcuts(const pvw_ctx* ctx, const uint64_t* noisy, size_t count, uint64_t* out_u64,
                                              uint8_t* short_path);
/* SELF-TEST (host only, no GPU): the per-context constants behind the short cuts of the device gadget decode
 * (decode_scalar_pvw_rns, src/crypto/decryption.rs:10-247: mixed-radix inverses and partial products of the leading
 * moduli, the normalised 2*Delta with its reciprocal, Delta^(l-1) mod q_i with its inverses) checked against their
 * defining identities.  info_out[0..3] = leading moduli used (0 = none), whether their mixed-radix digits reduce with one
 * subtraction, whether the chain runs on short operands, whether noise_{l-1} is proven without the Horner lift. */
PVW_API int32_t pvw_selftest_decode_tables(const pvw_ctx* ctx, uint32_t info_out[4]);
/* 1 for the measurement build libpvw_hip_tuning.so (include/pvw_hip_tuning.h: environment-selected kernel
 * schedules, timing ablations, bandwidth probe), 0 for the shipped library, which reads no environment variable */
PVW_API int32_t pvw_build_is_tuning(void);

/* ---- ring primitives (fhe-math call sites) -----------------------
 * change_representation(Ntt / PowerBasis) on `count` polynomials, host buffers, in place */
PVW_API int32_t pvw_ntt_forward(pvw_ctx* ctx, uint64_t* polys, size_t count);
PVW_API int32_t pvw_ntt_inverse(pvw_ctx* ctx, uint64_t* polys, size_t count);
/* Poly::from_coefficients(&[i64]) + NTT: coeffs [count][l] -> polys [count][L][l] */
PVW_API int32_t pvw_small_to_poly(pvw_ctx* ctx, const int64_t* coeffs, size_t count, uint64_t* polys,
                          uint32_t repr);

/* ---- samplers (src/sampling) on the device, counter-based, written to host ----------
 * polynomial p of the call uses stream (domain<<32) | (index0+p); out [count][l]. */
PVW_API int32_t pvw_sample_cbd(pvw_ctx* ctx, const uint8_t seed[32], uint32_t domain, uint32_t index0,
                       size_t count, float variance, int64_t* out);      /* uniform.rs:27-70 */
PVW_API int32_t pvw_sample_uniform(pvw_ctx* ctx, const uint8_t seed[32], uint32_t domain,
                           uint32_t index0, size_t count, uint64_t bound, int64_t* out); /* uniform.rs:5-22 */
PVW_API int32_t pvw_sample_gaussian(pvw_ctx* ctx, const uint8_t seed[32], uint32_t index0, size_t count,
                            uint64_t bound, int64_t* out /*[count]*/);    /* normal.rs:12-20,136-162 */

/* ---- Handover over a prime field of up to 256 bits: the public arithmetic either side of ONE pass of int64
 * combinations (pvw_ct_lincomb_many*, pvw_decrypt_all_lincomb_many_plain*), so that a committee moves its wide shares to a new
 * one with V decrypts a party instead of D NL.  Vector d NL + w is limb w of old holder d (the order pvw_deal_shares_wide*
 * writes).  A Lagrange weight of 256 bits cannot be an int64 weight, but |P| only has to stay below Q/2 (plain-modulus decode,
 * "Radius"), so mu_{d,w} = lambda_d 2^(limb_bits w) mod p is cut into V signed digits c_{d,w,v} of b = digit_bits bits, B = 2^b:
 *   P_v[j]       = sum_{d,w} c_{d,w,v} limb_{d,w}[j]      one combined ciphertext per digit, decrypted with wide_words = ww
 *   new share[j] = sum_v P_v[j] B^v mod p = sum_d lambda_d f_d(j + 1) mod p
 * The digit rule (host and device agree bit for bit): 8 <= b <= 64, V = ceil((bitlen(p) + 1) / b); for a value read mod p, x = its
 * centred residue in (-p/2, p/2]; for v = 0 .. V - 2: c_v = x mod B taken in [-B/2, B/2), x <- (x - c_v) / B; c_{V-1} = the
 * remaining x.  Every digit, the top one included, lies in [-2^(b-1), 2^(b-1)) and sum_v c_v B^v = x.  (The "+ 1" matters: with
 * ceil(bitlen(p) / b) digits the chain does not close, B = 4, V = 2, x = 6.)
 * plain_modulus is a HOST pointer to an odd prime below 2^256, checked as in the wide family; limb_bits follows
 * pvw_shamir_wide_limbs and gives NL.  Every refusal is PVW_ERR_INVALID_PARAMETERS before any device work, nothing written. */
/* NL and V of a field, a limb width and a digit width; host only */
PVW_API int32_t pvw_shamir_wide_handover_shape(const uint64_t* plain_modulus, uint32_t limb_bits, uint32_t digit_bits, uint32_t* num_limbs,
                                               uint32_t* num_digits);
/* digits [count][V] of values [count][4] (any words, read mod p) by the rule above; the device form runs the cut of the weights
 * kernel on device pointers, asynchronous on `stream`, allocates nothing, may be captured */
PVW_API int32_t pvw_shamir_wide_signed_digits_host(const uint64_t* plain_modulus, const uint64_t* values, size_t count, uint32_t digit_bits,
                                                   int64_t* digits);
PVW_API int32_t pvw_shamir_wide_signed_digits_device(pvw_ctx* ctx, const uint64_t* plain_modulus, const uint64_t* d_values, size_t count,
                                                     uint32_t digit_bits, int64_t* d_digits, void* stream);
/* The weight rows, weights [T V][D NL]: row m V + v, column d NL + w holds digit v of lambda_{d,m} 2^(limb_bits w) mod p, where
 * lambda_{.,m} are the Lagrange weights at points[m] over the points indices[d] + 1 of the VALID holders (valid [D] bytes, NULL =
 * all); every column of an invalid holder is 0.  points [T][4] below p, or NULL for the single point 0 (T = 1 then); the point
 * -m of a packed sharing is p - m.  A point equal to a valid holder's point gives that holder's unit vector (its columns hold
 * the digits of 2^(limb_bits w), all others 0); the point of an invalid holder is an ordinary point.  indices, valid and points
 * are HOST arrays in both forms, consumed at call time.  Refused: what pvw_shamir_reconstruct_wide refuses about the indices of
 * the valid holders, no valid holder, a point >= p, T = 0, digit_bits outside [8, 64], D NL >= 2^32, and T V >= 2^31 on the device.
 * The device form builds its public matrices in a block of the stream's workspace sized by the call: under stream capture it
 * needs an earlier call on that stream outside capture with at least as many valid holders and points. */
PVW_API int32_t pvw_shamir_wide_handover_weights_host(const uint64_t* plain_modulus, const uint64_t* indices, const uint8_t* valid,
                                                      size_t num_holders, const uint64_t* points, size_t num_points, uint32_t limb_bits,
                                                      uint32_t digit_bits, int64_t* weights);
PVW_API int32_t pvw_shamir_wide_handover_weights_device(pvw_ctx* ctx, const uint64_t* plain_modulus, const uint64_t* indices,
                                                        const uint8_t* valid, size_t num_holders, const uint64_t* points, size_t num_points,
                                                        uint32_t limb_bits, uint32_t digit_bits, int64_t* d_weights, void* stream);
/* The fold: out[i] = sum_v +-|P_{i,v}| B^v mod p, fully reduced, for wide [count][V][wide_words] and status [count][V] -- exactly
 * what pvw_decrypt_all_lincomb_many_plain* writes for R = T V rows, read in place with count = P T.  The sign is PVW_DEC_NEGATIVE
 * of status[i][v]; status_out[i] is the OR of the V words with PVW_DEC_NEGATIVE cleared (PVW_DEC_WIDE_TRUNCATED and the lossy bit
 * survive).  1 <= wide_words <= 4, 1 <= num_digits <= 33.  The device form: device pointers, asynchronous, may be captured. */
PVW_API int32_t pvw_shamir_wide_from_digits_host(const uint64_t* plain_modulus, uint32_t digit_bits, uint32_t num_digits,
                                                 const uint64_t* wide, uint32_t* status, uint32_t wide_words, size_t count,
                                                 uint64_t* out, uint32_t* status_out);
PVW_API int32_t pvw_shamir_wide_from_digits_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t digit_bits, uint32_t num_digits,
                                                   const uint64_t* d_wide, uint32_t* d_status, uint32_t wide_words, size_t count,
                                                   uint64_t* d_out, uint32_t* d_status_out, void* stream);
/* Every new party's new share in one call: out [P][T][4] (fully reduced) and status [P][T] for the parties [party_lo, party_hi),
 * P = party_hi - party_lo, from the old holders' limb ciphertexts c1s [D NL][k][L][l], c2s [D NL][n][L][l].  Behind the checks it
 * runs the device weights above, the body of pvw_decrypt_all_lincomb_many_plain* with R = T V rows over all D NL vectors
 * (valid = NULL there: a masked holder's weights are 0) and wide_words = ww = ceil((limb_bits + digit_bits +
 * ceil(log2(num_valid NL)) + 1) / 64), unchanged, and the fold above over its report in place.  out / status are bit for bit
 * pvw_shamir_wide_handover_weights_host -> that call -> pvw_shamir_wide_from_digits_host; *count (may be NULL) = the valid
 * holders.  Refused: NULL, what the weights call refuses, ww beyond the words of Q, what the many-combinations call refuses.
 * The digit plaintexts [P][R] are marked secret and cleared behind the fold (the weights and the combined ciphertexts are
 * public); the keys are staged and cleared by the many-combinations call.  The _device form takes device pointers for sk,
 * c1s, c2s, out, status and count (indices, valid, points and plain_modulus stay HOST arrays, consumed at call time) and is
 * asynchronous on `stream`; under stream capture it needs an earlier call outside capture on that stream with the same party
 * range and at least as many valid holders, rows T V and vectors (the rule of 8.15), and is refused with nothing enqueued
 * otherwise; a replay reads no host memory.  The host-buffer form may be called from several threads at once. */
PVW_API int32_t pvw_decrypt_all_handover_wide(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* sk, const uint64_t* c1s,
                                              const uint64_t* c2s, size_t num_dealers, const uint64_t* plain_modulus, uint32_t limb_bits,
                                              uint32_t digit_bits, const uint64_t* indices, const uint8_t* valid, const uint64_t* points,
                                              size_t num_points, uint32_t in_repr, uint64_t* out, uint32_t* status, uint32_t* count);
PVW_API int32_t pvw_decrypt_all_handover_wide_device(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const int64_t* d_sk,
                                                     const uint64_t* d_c1s, const uint64_t* d_c2s, size_t num_dealers,
                                                     const uint64_t* plain_modulus, uint32_t limb_bits, uint32_t digit_bits,
                                                     const uint64_t* indices, const uint8_t* valid, const uint64_t* points,
                                                     size_t num_points, uint32_t in_repr, uint64_t* d_out, uint32_t* d_status,
                                                     uint32_t* d_count, void* stream);
/* Advisory (host): *fits = 1 iff num_valid NL 2^(digit_bits - 1) pvw_ctx_noise_bound <= the radius of pvw_ctx_sum_capacity, and
 * ww = ceil((limb_bits + digit_bits + ceil(log2(num_valid NL)) + 1) / 64) is at most the words of Q.  Sufficient, not necessary,
 * like pvw_ctx_lincomb_fits; no entry point refuses on noise grounds. */
PVW_API int32_t pvw_ctx_wide_handover_fits(const pvw_ctx* ctx, const uint64_t* plain_modulus, size_t num_valid, uint32_t limb_bits,
                                           uint32_t digit_bits, uint32_t* fits);

/* ---- Wide share repair at field points: pvw_shamir_evaluate_wide_corrected* / _wide_erasures* (8.22) with the point
 * of every column of `values` given as a field element.  The arguments of the matching index form in its order, except that
 * `points`, `num_points` stand where it has `targets`, `num_targets`.
 *   points [num_points][4]: a HOST array of little-endian words in every form (like `points` in 8.24); the point of column j of
 *   values is points[j], which must be below p.  0, points above 2^64 and points that are some column's indices[c] + 1 are legal;
 *   duplicates and any order are allowed.
 *   out, nerr, col_err and err_mask are the decode-only call's, bit for bit.  values [num_secrets][num_points][4] follows 8.22's
 *   rule with x*_j = points[j]: at a point that equals indices[c] + 1 of a column the decode found right the share read mod p, on
 *   a wrong or erased column the share that party should hold, anywhere else F_s(x*_j); an undecodable row stores 0.
 *   With points[j] = targets[j] + 1 the call equals the index call on all five outputs, bit for bit; at points[j] = 0,
 *   values[s][j] = out[s].  erased == NULL is the corrected _at call bit for bit: behind the checks it is that call.  The three
 *   forms agree on every input.
 * PVW_ERR_INVALID_PARAMETERS before any device work, nothing written: what the matching index form refuses, with its texts and
 * in its order (the device bound r < 4096 included); then NULL points or values, num_points = 0, a point >= p; on the device
 * num_points >= 2^31, checked before the points are walked.
 * Under stream capture the rule of 8.22 unchanged, with num_points in the place of num_targets; the points travel as kernel
 * arguments (64 per launch), so a replay reads no host memory. */
PVW_API int32_t pvw_shamir_evaluate_wide_corrected_at_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                           size_t count, const uint64_t* shares, size_t num_secrets,
                                                           size_t secret_stride, size_t point_stride, const uint64_t* points,
                                                           size_t num_points, uint64_t* values, uint64_t* out, uint32_t* nerr,
                                                           uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_wide_corrected_at_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                             const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                             size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                             const uint64_t* points, size_t num_points, uint64_t* d_values,
                                                             uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                             uint64_t* d_err_mask, void* stream);
PVW_API int32_t pvw_shamir_evaluate_wide_corrected_at(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                      const uint64_t* indices, size_t count, const uint64_t* shares, size_t num_secrets,
                                                      size_t secret_stride, size_t point_stride, const uint64_t* points,
                                                      size_t num_points, uint64_t* values, uint64_t* out, uint32_t* nerr,
                                                      uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_wide_erasures_at_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                          size_t count, const uint64_t* shares, size_t num_secrets,
                                                          size_t secret_stride, size_t point_stride, const uint64_t* erased,
                                                          const uint64_t* points, size_t num_points, uint64_t* values, uint64_t* out,
                                                          uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_evaluate_wide_erasures_at_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                            const uint64_t* indices, size_t count, const uint64_t* d_shares,
                                                            size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                            const uint64_t* d_erased, const uint64_t* points, size_t num_points,
                                                            uint64_t* d_values, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                            uint64_t* d_err_mask, void* stream);
PVW_API int32_t pvw_shamir_evaluate_wide_erasures_at(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t degree,
                                                     const uint64_t* indices, size_t count, const uint64_t* shares, size_t num_secrets,
                                                     size_t secret_stride, size_t point_stride, const uint64_t* erased,
                                                     const uint64_t* points, size_t num_points, uint64_t* values, uint64_t* out,
                                                     uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);
/* The secrets of packed wide rows (8.23) in one call, with shares wrong or erased.  degree = t, the number of random coefficients,
 * as in pvw_shamir_shares_packed_wide*: a row is decoded at polynomial degree t + pack - 1 with r = count - t - pack and decodes
 * while 2 errors + erasures <= r.  secrets [num_rows][pack][4]: secrets[s][m] = F_s(-m), fully reduced; a row reported
 * PVW_SHAMIR_UNDECODABLE gives `pack` zero elements.  erased may be NULL; nerr, col_err, err_mask as the wide erasures call at
 * that degree reports them, each optional.  pack = 1 is pvw_shamir_reconstruct_wide_erasures* on secrets and all three reports.
 * Refused (PVW_ERR_INVALID_PARAMETERS, nothing written): NULL plain_modulus, indices, shares or secrets; pack = 0 or
 * pack > PVW_WIDE_MAX_PACK; count < degree + pack and everything else the wide erasures call refuses at degree + pack - 1; an
 * index >= p - pack (the rule of pvw_shamir_reconstruct_packed_wide: no secret point meets a column).
 * Behind the checks it is the evaluation above with num_points = pack and `secrets` its values.  The _device form makes the
 * points p - m on the device and takes no host array of points, so it captures like the decode: an earlier call of this kind on
 * that stream outside capture with the same degree, pack and count, at least as many rows, and a mask if this one has one. */
PVW_API int32_t pvw_shamir_packed_wide_secrets_host(const uint64_t* plain_modulus, uint32_t pack, uint32_t degree, const uint64_t* indices,
                                                    size_t count, const uint64_t* shares, size_t num_rows, size_t secret_stride,
                                                    size_t point_stride, const uint64_t* erased, uint64_t* secrets, uint32_t* nerr,
                                                    uint32_t* col_err, uint64_t* err_mask);
PVW_API int32_t pvw_shamir_packed_wide_secrets_device(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t pack, uint32_t degree,
                                                      const uint64_t* indices, size_t count, const uint64_t* d_shares, size_t num_rows,
                                                      size_t secret_stride, size_t point_stride, const uint64_t* d_erased,
                                                      uint64_t* d_secrets, uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask,
                                                      void* stream);
PVW_API int32_t pvw_shamir_packed_wide_secrets(pvw_ctx* ctx, const uint64_t* plain_modulus, uint32_t pack, uint32_t degree,
                                               const uint64_t* indices, size_t count, const uint64_t* shares, size_t num_rows,
                                               size_t secret_stride, size_t point_stride, const uint64_t* erased, uint64_t* secrets,
                                               uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask);

/* ---- measurement hooks -------------------------------------------------------------
 * With profiling on, every kernel launch of the context is bracketed by HIP events on
 * its stream; pvw_ctx_kernel_time returns the accumulated device time of kernel `name`
 * ("mac_rows", "prep", "sample", "intt", "decrypt_mac", ...) and resets nothing. */
PVW_API int32_t pvw_ctx_set_profiling(pvw_ctx* ctx, int32_t on);
PVW_API int32_t pvw_ctx_kernel_time(pvw_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);
PVW_API int32_t pvw_ctx_reset_profiling(pvw_ctx* ctx);
/* Host memory the device can write directly (pinned + mapped).  pvw_encrypt recognises output buffers that live in
 * such memory -- from here, or pinned / registered by the caller (hipHostMalloc, hipHostRegister) -- and, for
 * PVW_REPR_NTT output, has the kernel store c1 / c2 straight into them while it runs: the ciphertexts (4.7 MB at
 * n = 4096, k = 256, 1037-bit q) cross PCIe under the kernel instead of in a copy after it.  Pageable buffers work as
 * before.  (encryption.rs:105 returns host objects; a Rust host allocates the Vec it converts from with this.) */
PVW_API int32_t pvw_host_alloc(size_t bytes, void** out);
PVW_API int32_t pvw_host_free(void* p);

/* geometry of the resident tensors (bytes) for roofline bookkeeping: the tiled A-hat / B-hat sections ... */
PVW_API int32_t pvw_ctx_resident_bytes(const pvw_ctx* ctx, uint64_t* crs_bytes, uint64_t* pk_bytes);
/* ... and the derived copies held next to them at the moment (0 when not built) */
PVW_API int32_t pvw_ctx_derived_bytes(const pvw_ctx* ctx, uint64_t* packed_bytes, uint64_t* mfma_tiled_bytes);

/* ---- derived copies as an explicit step (GlobalPublicKey's mutators take &mut self, src/keys/public_key.rs:214-263:
 * in the reference a key change and an encrypt never overlap, so there is a well-defined moment for this) -------------
 * pvw_prepare builds, NOW and on `stream` (NULL = the context's own), what later *_device calls on that stream would
 * otherwise build lazily: the stream's workspace, and for
 *   PVW_PREPARE_PACKED  the bit-packed copies of A-hat / B-hat that single-dealer encrypt streams (encryption.rs:177-200):
 *                       40 / 48 / 56 / 61 bits per residue by the widest modulus; l <= 16, k a multiple of 64 (256 at
 *                       61 bits); skipped -- not an error -- when the geometry does not qualify or memory is short
 *                       (pvw_ctx_packed_active tells; the tiled matrices are streamed then, and the allocation is
 *                       retried by later encrypts every so often);
 *   PVW_PREPARE_MFMA    the MFMA-tiled copies and digit buffers of multi-dealer encrypt (encryption.rs:253-286);
 *   PVW_PREPARE_SUM     the scratch of the pvw_ct_sum_device / pvw_decrypt_sum_* / pvw_decrypt_all_sum_{checked,plain}_device calls (the
 *                       slice sums, the summed ciphertext, and the decrypt scratch for the context's own party range); needs
 *                       no CRS and builds no copy.
 * It allocates, waits for the builds, and returns the bytes it allocated for the copies in *bytes_out (may be NULL).
 * Any later pvw_load_crs* / pvw_load_pk* / pvw_keygen / pvw_*_generate / fill invalidates the copies of the matrix it
 * touched; call pvw_prepare again (only that matrix's copies are rebuilt; nothing is reallocated). */
enum { PVW_PREPARE_PACKED = 1, PVW_PREPARE_MFMA = 2, PVW_PREPARE_SUM = 4 };
PVW_API int32_t pvw_prepare(pvw_ctx* ctx, uint32_t flags, void* stream, uint64_t* bytes_out);
/* the stream single-dealer encrypt would use right now: *width_out = bits per residue of the valid packed copies,
 * 0 = the tiled matrices (copies not built, invalidated, geometry not eligible, or no room) */
PVW_API int32_t pvw_ctx_packed_active(const pvw_ctx* ctx, uint32_t* width_out);
PVW_API int32_t pvw_ctx_synchronize(pvw_ctx* ctx);

/* ---- wire format, version 1: this library's own byte form of parameters, CRS rows, public-key rows, ciphertexts
 * and secret keys (the reference serialises them through serde, encryption.rs:298-354, public_key.rs:471-622, crs.rs:228-295,
 * parameters.rs:606-664; its fhe-math Poly bytes are not reproducible here).  A blob is a header that carries the parameters
 * and a body.  A packed polynomial holds limb row i at w_i = bitlen(q_i) bits per residue, least significant bit first, rows
 * back to back: pvw_wire_poly_bytes = (l/8) * sum_i w_i, and polynomial p of a body starts at byte p * poly_bytes.
 *   Writers emit w mod q_i for every word w (unreduced and reduced words give the same bytes).  Readers reject any field >= q_i
 *   with PVW_ERR_DESERIALIZATION; the message names the first bad polynomial, limb and slot.
 *   Kinds: 1 parameters (no body), 2 CRS rows, 3 public-key rows (row = k polynomials), 4 ciphertext (c1 rows then c2 rows),
 *   5 secret key (k*l int64, not packed).  The device codec takes L <= 64 moduli and 16-byte aligned device pointers. */
PVW_API int32_t pvw_wire_poly_bytes(const pvw_ctx* ctx, size_t* out);
/* the header of a blob of `kind` for this context: rows [lo, hi) (kinds 2 / 3), c1 rows [lo, hi) and c2 rows [lo2, hi2) (kind 4);
 * unused range arguments are ignored.  *len = header length (a multiple of 16); out = NULL only reports it.  cap < *len:
 * PVW_ERR_SERIALIZATION.  Ranges beyond the parameters: PVW_ERR_INVALID_FORMAT. */
PVW_API int32_t pvw_wire_header(const pvw_ctx* ctx, uint32_t kind, uint32_t repr, uint32_t lo, uint32_t hi, uint32_t lo2,
                                uint32_t hi2, uint8_t* out, size_t cap, size_t* len);
/* checks a whole blob (header + body, len bytes) against this context.  Wrong magic, version, kind or representation,
 * other moduli / variance / bounds, other roots for an NTT-domain body, bad ranges, a body_len that does not match, a
 * truncated blob or trailing bytes: PVW_ERR_INVALID_FORMAT; other n / k / l / L: PVW_ERR_DIMENSION_MISMATCH.  Outputs (each
 * may be NULL): kind, repr, ranges[4] = {lo, hi, lo2, hi2} (0 where unused), header_len (the body starts there). */
PVW_API int32_t pvw_wire_header_check(const pvw_ctx* ctx, const uint8_t* data, size_t len, uint32_t* kind, uint32_t* repr,
                                      uint32_t* ranges, size_t* header_len);
/* `count` polynomials [L][l] <-> count * poly_bytes packed bytes, host buffers, on the device (synchronous).  pack: `out` may
 * be pvw_host_alloc memory, which the kernel then writes directly.  unpack: on rejection polys is written all the same. */
PVW_API int32_t pvw_wire_pack(pvw_ctx* ctx, const uint64_t* polys, size_t count, uint8_t* out);
PVW_API int32_t pvw_wire_pack_device(pvw_ctx* ctx, const uint64_t* d_polys, size_t count, uint8_t* d_out, void* stream);
PVW_API int32_t pvw_wire_unpack(pvw_ctx* ctx, const uint8_t* data, size_t count, uint64_t* polys);
/* asynchronous on `stream`, no host synchronisation (may be captured): *d_bad (device word) = the number of rejected residues;
 * rejected slots hold the raw field value.  d_out of pack may be pvw_host_alloc memory. */
PVW_API int32_t pvw_wire_unpack_device(pvw_ctx* ctx, const uint8_t* d_in, size_t count, uint64_t* d_polys, uint64_t* d_bad,
                                       void* stream);
/* the same codec in plain C++ on the host (no GPU needed): the reference the device codec is tested against.
 * unpack_host: *bad_out (may be NULL) = rejected residues; PVW_ERR_DESERIALIZATION if any. */
PVW_API int32_t pvw_wire_pack_host(const pvw_ctx* ctx, const uint64_t* polys, size_t count, uint8_t* out);
PVW_API int32_t pvw_wire_unpack_host(const pvw_ctx* ctx, const uint8_t* data, size_t count, uint64_t* polys, uint64_t* bad_out);
/* pvw_load_pk / pvw_load_crs from a packed body (rows [party_lo, party_hi) / [0, k); rows outside the context's shard are not
 * read).  Every row the context holds is checked before any is stored: a rejected body (PVW_ERR_DESERIALIZATION) leaves the
 * resident matrix, num_public_keys and the derived copies as they were.  Bodies up to 1 GiB are staged on the device whole,
 * larger ones are read twice.  On success the derived copies are invalidated as by pvw_load_pk / pvw_load_crs. */
PVW_API int32_t pvw_load_pk_wire(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, const uint8_t* body, uint32_t repr);
/* pvw_get_pk / pvw_get_crs packed: untiled (and transformed for POWER) and packed on the device, only the packed bytes are
 * copied to the host.  Rows the context does not hold are not written. */
PVW_API int32_t pvw_get_pk_wire(pvw_ctx* ctx, uint32_t party_lo, uint32_t party_hi, uint8_t* body_out, uint32_t repr);
PVW_API int32_t pvw_load_crs_wire(pvw_ctx* ctx, const uint8_t* body, uint32_t repr);
PVW_API int32_t pvw_get_crs_wire(pvw_ctx* ctx, uint8_t* body_out, uint32_t repr);

#ifdef __cplusplus
}
#endif
#endif /* PVW_HIP_H */

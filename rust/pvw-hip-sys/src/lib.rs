//! Raw bindings to `libpvw_hip.so` -- one to one with `include/pvw_hip.h`.
//!
//! **NOT COMPILED in this repository's pipeline** (no Rust toolchain in the image; see `rust/README.md`).
//! `tests/test_rust_binding.py` keeps this file honest: it parses the header and the `extern "C"` block below and
//! asserts the same symbol set, arity and argument widths, the `#[repr(C)]` field order and the status codes.
//!
//! Conventions (details in the header): every function returns `i32` (0 = `PVW_OK`, otherwise the 1-based index of
//! the `PvwError` variant in declaration order, `src/errors.rs:13-70`; the message is `pvw_last_error`, thread
//! local); a polynomial is `[L][l]` `u64`, limb-major (`src/params/parameters.rs:433-458`); host-buffer calls are
//! synchronous and may be issued concurrently on one context (rayon does, `src/crypto/encryption.rs:277-283`);
//! `*_device` calls take device pointers and a `hipStream_t` and only enqueue.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_void};

/// Opaque device context behind one `PvwParameters` (`pvw_ctx` in the header).
#[repr(C)]
pub struct PvwCtx {
    _private: [u8; 0],
}

/// Opaque device-resident secret key (`pvw_sk` in the header): NTT(sk) as the inner products of decrypt read it.
#[repr(C)]
pub struct PvwSk {
    _private: [u8; 0],
}

/// `pvw_params_t`: the `PvwParametersBuilder` fields (`src/params/parameters.rs:44-52`) plus device placement.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct PvwParamsT {
    pub n: u32,
    pub k: u32,
    pub l: u32,
    pub num_moduli: u32,
    pub moduli: *const u64,
    pub secret_variance: f32,
    pub error_bound_1: u64,
    pub error_bound_2: u64,
    pub device: i32,
    pub party_lo: u32,
    pub party_hi: u32,
    pub c1_lo: u32,
    pub c1_hi: u32,
}

/// `pvw_randomness_t`: the randomness of one encrypt call (the reference draws from `thread_rng()` inside rayon
/// closures, `src/crypto/encryption.rs:138,164,180`, which cannot cross an FFI boundary).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct PvwRandomnessT {
    pub mode: u32,
    pub seed: [u8; 32],
    pub r: *const i64,
    pub e1: *const i64,
    pub e2: *const i64,
}

pub const PVW_PREPARE_PACKED: u32 = 1;
pub const PVW_PREPARE_MFMA: u32 = 2;
pub const PVW_PREPARE_SUM: u32 = 4;
/// status bit of the checked decrypt: the returned word is not the plaintext (pvw_hip.h)
pub const PVW_DEC_LOSSY: u32 = 1;
pub const PVW_DEC_NEGATIVE: u32 = 2;
pub const PVW_DEC_WIDE_TRUNCATED: u32 = 4;
pub const PVW_OK: i32 = 0;
pub const PVW_ERR_INVALID_PARAMETERS: i32 = 1;
pub const PVW_ERR_SAMPLING: i32 = 2;
pub const PVW_ERR_ENCRYPTION: i32 = 3;
pub const PVW_ERR_DECRYPTION: i32 = 4;
pub const PVW_ERR_KEY_GENERATION: i32 = 5;
pub const PVW_ERR_CRS: i32 = 6;
pub const PVW_ERR_SERIALIZATION: i32 = 7;
pub const PVW_ERR_DESERIALIZATION: i32 = 8;
pub const PVW_ERR_ENCODING: i32 = 9;
pub const PVW_ERR_DECODING: i32 = 10;
pub const PVW_ERR_VALIDATION: i32 = 11;
pub const PVW_ERR_CONTEXT: i32 = 12;
pub const PVW_ERR_POLYNOMIAL: i32 = 13;
pub const PVW_ERR_MATRIX: i32 = 14;
pub const PVW_ERR_DIMENSION_MISMATCH: i32 = 15;
pub const PVW_ERR_INDEX_OUT_OF_BOUNDS: i32 = 16;
pub const PVW_ERR_INSUFFICIENT_DATA: i32 = 17;
pub const PVW_ERR_INVALID_FORMAT: i32 = 18;
pub const PVW_ERR_INTERNAL: i32 = 19;

pub const PVW_REPR_POWER: u32 = 0;
pub const PVW_REPR_NTT: u32 = 1;
pub const PVW_RND_SEED: u32 = 0;
pub const PVW_RND_EXPLICIT: u32 = 1;

pub const PVW_DOM_R: u32 = 0;
pub const PVW_DOM_E1: u32 = 1;
pub const PVW_DOM_E2: u32 = 2;
pub const PVW_DOM_SK: u32 = 3;
pub const PVW_DOM_EKEY: u32 = 4;
pub const PVW_DOM_CRS: u32 = 5;
pub const PVW_DOM_GAUSS: u32 = 6;
pub const PVW_DOM_PK: u32 = 7;
pub const PVW_DOM_CALL: u32 = 8;
pub const PVW_DOM_SHAMIR: u32 = 9;
/// `nerr` of a secret that no polynomial of the degree fits within E columns
pub const PVW_SHAMIR_UNDECODABLE: u32 = 0xFFFF_FFFF;
/// the device forms of `pvw_shamir_reconstruct_wide_corrected` take at most this many locator coefficients
pub const PVW_SHAMIR_WIDE_MAX_LOCATOR: u32 = 2048;

extern "C" {
    // ---- errors / device ------------------------------------------------------------------
    pub fn pvw_last_error(buf: *mut c_char, len: usize) -> i32;
    pub fn pvw_device_available() -> i32;
    // ---- parameters: PvwParametersBuilder::build (src/params/parameters.rs:117-195) --------
    pub fn pvw_ctx_create(params: *const PvwParamsT, out: *mut *mut PvwCtx) -> i32;
    pub fn pvw_ctx_destroy(ctx: *mut PvwCtx) -> i32;
    pub fn pvw_ctx_get_roots(ctx: *const PvwCtx, psi_out: *mut u64) -> i32;
    pub fn pvw_ctx_set_roots(ctx: *mut PvwCtx, psi: *const u64) -> i32;
    pub fn pvw_ctx_delta(ctx: *const PvwCtx, words: *mut u64, cap: usize, nwords: *mut usize) -> i32;
    pub fn pvw_ctx_delta_power_l_minus_1(ctx: *const PvwCtx, words: *mut u64, cap: usize, nwords: *mut usize) -> i32;
    pub fn pvw_ctx_q_total(ctx: *const PvwCtx, words: *mut u64, cap: usize, nwords: *mut usize) -> i32;
    pub fn pvw_ctx_gadget(ctx: *const PvwCtx, poly_out: *mut u64, repr: u32) -> i32;
    pub fn pvw_ctx_verify_correctness_condition(ctx: *const PvwCtx, ok_out: *mut i32) -> i32;
    pub fn pvw_suggest_error_bounds(n: u32, k: u32, l: u32, moduli: *const u64, num_moduli: u32, variance: f32, bound1_out: *mut u32, bound2_out: *mut u32) -> i32;
    pub fn pvw_encode_scalar(ctx: *const PvwCtx, scalar: i64, poly_out: *mut u64, repr: u32) -> i32;
    // ---- CRS: PvwCrs.matrix (src/params/crs.rs:12-17), constructors :24-90 -------------------
    pub fn pvw_load_crs(ctx: *mut PvwCtx, a: *const u64, repr: u32) -> i32;
    pub fn pvw_load_crs_device(ctx: *mut PvwCtx, d_a: *const u64, repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_crs_generate(ctx: *mut PvwCtx, seed: *const u8) -> i32;
    pub fn pvw_crs_seed_from_tag(tag: *const c_char, seed_out: *mut u8) -> i32;
    pub fn pvw_get_crs(ctx: *mut PvwCtx, a_out: *mut u64, repr: u32) -> i32;
    // ---- global public key: GlobalPublicKey.matrix (src/keys/public_key.rs:43-54, :214-250) --
    pub fn pvw_load_pk(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, b: *const u64, repr: u32) -> i32;
    pub fn pvw_load_pk_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_b: *const u64, repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_pk_fill_uniform(ctx: *mut PvwCtx, seed: *const u8) -> i32;
    pub fn pvw_get_pk(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, b_out: *mut u64, repr: u32) -> i32;
    pub fn pvw_num_public_keys(ctx: *const PvwCtx, out: *mut u32) -> i32;
    pub fn pvw_is_full(ctx: *const PvwCtx, out: *mut i32) -> i32;
    // ---- key generation: PublicKey::generate (public_key.rs:111-147) over crs.rs:138-171 ------
    pub fn pvw_keygen(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, ek: *const i64, seed: *const u8) -> i32;
    pub fn pvw_sample_secret_keys(ctx: *const PvwCtx, seed: *const u8, party_lo: u32, count: u32, sk_out: *mut i64) -> i32;
    pub fn pvw_keygen_seeded(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk_seed: *const u8, seed: *const u8) -> i32;
    pub fn pvw_sample_secret_keys_device(ctx: *mut PvwCtx, seed: *const u8, party_lo: u32, count: u32, d_sk_out: *mut i64, stream: *mut c_void) -> i32;
    // ---- encrypt (src/crypto/encryption.rs:105-214), encrypt_all_party_shares (:253-286) ------
    pub fn pvw_encrypt(ctx: *mut PvwCtx, scalars: *const u64, num_scalars: usize, rnd: *const PvwRandomnessT, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_encrypt_device(ctx: *mut PvwCtx, d_scalars: *const u64, num_scalars: usize, rnd: *const PvwRandomnessT, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_encrypt_multi(ctx: *mut PvwCtx, scalars: *const u64, num_dealers: usize, scalars_per_dealer: usize, seeds: *const u8, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_encrypt_multi_device(ctx: *mut PvwCtx, d_scalars: *const u64, num_dealers: usize, scalars_per_dealer: usize, seeds: *const u8, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    // ---- encrypt from a device randomness state (an opaque handle: seed + counter on the device) ----
    pub fn pvw_rnd_state_create(ctx: *mut PvwCtx, seed: *const u8, counter: u64, out: *mut *mut c_void) -> i32;
    pub fn pvw_rnd_state_counter(st: *mut c_void, stream: *mut c_void, out: *mut u64) -> i32;
    pub fn pvw_rnd_state_set_counter(st: *mut c_void, counter: u64, stream: *mut c_void) -> i32;
    pub fn pvw_rnd_state_free(st: *mut c_void) -> i32;
    pub fn pvw_rnd_call_seed(seed: *const u8, counter: u64, out: *mut u8) -> i32;
    pub fn pvw_encrypt_rs(ctx: *mut PvwCtx, scalars: *const u64, num_scalars: usize, st: *mut c_void, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_encrypt_rs_device(ctx: *mut PvwCtx, d_scalars: *const u64, num_scalars: usize, st: *mut c_void, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_encrypt_multi_rs(ctx: *mut PvwCtx, scalars: *const u64, num_dealers: usize, scalars_per_dealer: usize, st: *mut c_void, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_encrypt_multi_rs_device(ctx: *mut PvwCtx, d_scalars: *const u64, num_dealers: usize, scalars_per_dealer: usize, st: *mut c_void, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    // ---- Shamir shares ------------------------------------------------------------
    pub fn pvw_shamir_shares_host(ctx: *const PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_shamir_shares_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, seeds: *const u8, d_coeffs: *const u64, d_shares: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_shares(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_deal_shares(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, seeds: *const u8, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, seeds: *const u8, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_deal_shares_rs(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, st: *mut c_void, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_rs_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: u64, st: *mut c_void, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct(plain_modulus: u64, indices: *const u64, shares: *const u64, count: usize, num_secrets: usize, out: *mut u64) -> i32;
    // ---- packed sharing ------------------------------------------------------------
    // Shamir shares over a prime below 2^256: plain_modulus points at four words
    pub fn pvw_shamir_wide_limbs(plain_modulus: *const u64, limb_bits: u32, num_limbs: *mut u32) -> i32;
    pub fn pvw_shamir_shares_wide_host(ctx: *const PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_shamir_shares_wide_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, seeds: *const u8, d_coeffs: *const u64, d_shares: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_shares_wide(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_deal_shares_wide(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, limb_bits: u32, seeds: *const u8, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_wide_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, limb_bits: u32, seeds: *const u8, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_deal_shares_wide_rs(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, limb_bits: u32, st: *mut c_void, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_wide_rs_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, degree: u32, plain_modulus: *const u64, limb_bits: u32, st: *mut c_void, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_wide_to_limbs_host(values: *const u64, count: usize, limb_bits: u32, num_limbs: u32, limbs_out: *mut u64) -> i32;
    pub fn pvw_shamir_wide_from_limbs_host(plain_modulus: *const u64, limbs: *const u64, count: usize, limb_bits: u32, num_limbs: u32, out: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_wide(plain_modulus: *const u64, indices: *const u64, shares: *const u64, count: usize, num_secrets: usize, out: *mut u64) -> i32;
    pub fn pvw_selftest_shamir_wide_step(ctx: *mut PvwCtx, plain_modulus: *const u64, acc: *const u64, x: *const u64, add: *const u64, count: usize, out: *mut u64) -> i32;
    // ---- packed sharing over a prime below 2^256: secrets [D][pack][4] ----
    pub fn pvw_shamir_shares_packed_wide_host(ctx: *const PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_shamir_shares_packed_wide_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, seeds: *const u8, d_coeffs: *const u64, d_shares: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_shares_packed_wide(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_deal_shares_packed_wide(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, limb_bits: u32, seeds: *const u8, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_packed_wide_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, limb_bits: u32, seeds: *const u8, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_deal_shares_packed_wide_rs(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, limb_bits: u32, st: *mut c_void, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_packed_wide_rs_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: *const u64, limb_bits: u32, st: *mut c_void, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_packed_wide(plain_modulus: *const u64, pack: u32, indices: *const u64, shares: *const u64, count: usize, num_rows: usize, out: *mut u64) -> i32;
    // ---- handover over a prime below 2^256: weight rows of signed digits, the fold of the digit plaintexts ----
    pub fn pvw_shamir_wide_handover_shape(plain_modulus: *const u64, limb_bits: u32, digit_bits: u32, num_limbs: *mut u32, num_digits: *mut u32) -> i32;
    pub fn pvw_shamir_wide_signed_digits_host(plain_modulus: *const u64, values: *const u64, count: usize, digit_bits: u32, digits: *mut i64) -> i32;
    pub fn pvw_shamir_wide_signed_digits_device(ctx: *mut PvwCtx, plain_modulus: *const u64, d_values: *const u64, count: usize, digit_bits: u32, d_digits: *mut i64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_wide_handover_weights_host(plain_modulus: *const u64, indices: *const u64, valid: *const u8, num_holders: usize, points: *const u64, num_points: usize, limb_bits: u32, digit_bits: u32, weights: *mut i64) -> i32;
    pub fn pvw_shamir_wide_handover_weights_device(ctx: *mut PvwCtx, plain_modulus: *const u64, indices: *const u64, valid: *const u8, num_holders: usize, points: *const u64, num_points: usize, limb_bits: u32, digit_bits: u32, d_weights: *mut i64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_wide_from_digits_host(plain_modulus: *const u64, digit_bits: u32, num_digits: u32, wide: *const u64, status: *mut u32, wide_words: u32, count: usize, out: *mut u64, status_out: *mut u32) -> i32;
    pub fn pvw_shamir_wide_from_digits_device(ctx: *mut PvwCtx, plain_modulus: *const u64, digit_bits: u32, num_digits: u32, d_wide: *const u64, d_status: *mut u32, wide_words: u32, count: usize, d_out: *mut u64, d_status_out: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_handover_wide(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, plain_modulus: *const u64, limb_bits: u32, digit_bits: u32, indices: *const u64, valid: *const u8, points: *const u64, num_points: usize, in_repr: u32, out: *mut u64, status: *mut u32, count: *mut u32) -> i32;
    pub fn pvw_decrypt_all_handover_wide_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, plain_modulus: *const u64, limb_bits: u32, digit_bits: u32, indices: *const u64, valid: *const u8, points: *const u64, num_points: usize, in_repr: u32, d_out: *mut u64, d_status: *mut u32, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_ctx_wide_handover_fits(ctx: *const PvwCtx, plain_modulus: *const u64, num_valid: usize, limb_bits: u32, digit_bits: u32, fits: *mut u32) -> i32;
    // ---- the one-word handover from a mask that may be made on the device ----
    pub fn pvw_shamir_handover_weights_host(plain_modulus: u64, indices: *const u64, valid: *const u8, num_holders: usize, targets: *const u64, num_targets: usize, weights: *mut i64, count: *mut u32) -> i32;
    pub fn pvw_shamir_handover_weights_device(ctx: *mut PvwCtx, plain_modulus: u64, indices: *const u64, d_valid: *const u8, num_holders: usize, targets: *const u64, num_targets: usize, d_weights: *mut i64, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_valid_mask_host(status: *mut u32, noise: *const u64, status_bits: u32, noise_bound: u64, count: usize, rows: usize, row_stride: usize, col_stride: usize, valid_out: *mut u8, num_valid: *mut u32) -> i32;
    pub fn pvw_shamir_valid_mask_device(ctx: *mut PvwCtx, d_status: *mut u32, d_noise: *const u64, status_bits: u32, noise_bound: u64, count: usize, rows: usize, row_stride: usize, col_stride: usize, d_valid_out: *mut u8, d_num_valid: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_handover(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_holders: usize, valid: *const u8, indices: *const u64, targets: *const u64, num_targets: usize, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_all_handover_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_holders: usize, d_valid: *const u8, indices: *const u64, targets: *const u64, num_targets: usize, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    // ---- the receiving end over a prime below 2^256: device fold of limbs, checked reconstruction ----
    pub fn pvw_shamir_wide_from_limbs_device(ctx: *mut PvwCtx, plain_modulus: *const u64, d_limbs: *const u64, count: usize, limb_stride: usize, elem_stride: usize, limb_bits: u32, num_limbs: u32, d_out: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_wide_checked_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, bad: *mut u32, col_bad: *mut u32) -> i32;
    pub fn pvw_shamir_reconstruct_wide_checked_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_out: *mut u64, d_bad: *mut u32, d_col_bad: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_wide_checked(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, bad: *mut u32, col_bad: *mut u32) -> i32;
    pub fn pvw_shamir_reconstruct_wide_corrected_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_wide_corrected_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_wide_corrected(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_selftest_shamir_wide_mul(ctx: *mut PvwCtx, plain_modulus: *const u64, a: *const u64, b: *const u64, count: usize, out: *mut u64) -> i32;
    pub fn pvw_shamir_shares_packed_host(ctx: *const PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_shamir_shares_packed_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, seeds: *const u8, d_coeffs: *const u64, d_shares: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_shares_packed(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, seeds: *const u8, coeffs: *const u64, shares_out: *mut u64) -> i32;
    pub fn pvw_deal_shares_packed(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, seeds: *const u8, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_packed_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, seeds: *const u8, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_deal_shares_packed_rs(ctx: *mut PvwCtx, secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, st: *mut c_void, c1_out: *mut u64, c2_out: *mut u64, out_repr: u32) -> i32;
    pub fn pvw_deal_shares_packed_rs_device(ctx: *mut PvwCtx, d_secrets: *const u64, num_dealers: usize, pack: u32, degree: u32, plain_modulus: u64, st: *mut c_void, d_c1: *mut u64, d_c2: *mut u64, out_repr: u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_packed(plain_modulus: u64, pack: u32, indices: *const u64, shares: *const u64, count: usize, num_rows: usize, out: *mut u64) -> i32;
    // ---- checked reconstruction --------------------------------------------------
    pub fn pvw_shamir_reconstruct_checked_host(plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, bad: *mut u32, col_bad: *mut u32) -> i32;
    pub fn pvw_shamir_reconstruct_checked_device(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_out: *mut u64, d_bad: *mut u32, d_col_bad: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_checked(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, bad: *mut u32, col_bad: *mut u32) -> i32;
    // ---- corrected reconstruction ------------------------------------------------
    pub fn pvw_shamir_reconstruct_corrected_host(plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_corrected_device(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    // ---- share repair --------------------------------------------------------------
    pub fn pvw_shamir_evaluate_corrected_host(plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_corrected_device(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, targets: *const u64, num_targets: usize, d_values: *mut u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_evaluate_corrected(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_corrected(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    // ---- reconstruction with erasures ----------------------------------------------
    pub fn pvw_shamir_reconstruct_erasures_host(plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_erasures_device(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_erased: *const u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_erasures(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_erasures_host(plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_erasures_device(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_erased: *const u64, targets: *const u64, num_targets: usize, d_values: *mut u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_evaluate_erasures(ctx: *mut PvwCtx, plain_modulus: u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_wide_erasures_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_reconstruct_wide_erasures_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_erased: *const u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_reconstruct_wide_erasures(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_corrected_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_corrected_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, targets: *const u64, num_targets: usize, d_values: *mut u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_evaluate_wide_corrected(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_erasures_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_erasures_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_erased: *const u64, targets: *const u64, num_targets: usize, d_values: *mut u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_evaluate_wide_erasures(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, targets: *const u64, num_targets: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_corrected_at_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, points: *const u64, num_points: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_corrected_at_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, points: *const u64, num_points: usize, d_values: *mut u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_evaluate_wide_corrected_at(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, points: *const u64, num_points: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_erasures_at_host(plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, points: *const u64, num_points: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_evaluate_wide_erasures_at_device(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, d_erased: *const u64, points: *const u64, num_points: usize, d_values: *mut u64, d_out: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_evaluate_wide_erasures_at(ctx: *mut PvwCtx, plain_modulus: *const u64, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_secrets: usize, secret_stride: usize, point_stride: usize, erased: *const u64, points: *const u64, num_points: usize, values: *mut u64, out: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_packed_wide_secrets_host(plain_modulus: *const u64, pack: u32, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_rows: usize, secret_stride: usize, point_stride: usize, erased: *const u64, secrets: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_packed_wide_secrets_device(ctx: *mut PvwCtx, plain_modulus: *const u64, pack: u32, degree: u32, indices: *const u64, count: usize, d_shares: *const u64, num_rows: usize, secret_stride: usize, point_stride: usize, d_erased: *const u64, d_secrets: *mut u64, d_nerr: *mut u32, d_col_err: *mut u32, d_err_mask: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_packed_wide_secrets(ctx: *mut PvwCtx, plain_modulus: *const u64, pack: u32, degree: u32, indices: *const u64, count: usize, shares: *const u64, num_rows: usize, secret_stride: usize, point_stride: usize, erased: *const u64, secrets: *mut u64, nerr: *mut u32, col_err: *mut u32, err_mask: *mut u64) -> i32;
    pub fn pvw_shamir_wide_erasure_mask_host(status: *mut u32, noise: *const u64, status_bits: u32, noise_bound: u64, count: usize, num_secrets: usize, secret_stride: usize, point_stride: usize, num_limbs: u32, limb_stride: usize, mask_out: *mut u64) -> i32;
    pub fn pvw_shamir_wide_erasure_mask_device(ctx: *mut PvwCtx, d_status: *mut u32, d_noise: *const u64, status_bits: u32, noise_bound: u64, count: usize, num_secrets: usize, secret_stride: usize, point_stride: usize, num_limbs: u32, limb_stride: usize, d_mask_out: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_shamir_erasure_mask_host(status: *mut u32, noise: *const u64, status_bits: u32, noise_bound: u64, count: usize, num_secrets: usize, secret_stride: usize, point_stride: usize, mask_out: *mut u64) -> i32;
    pub fn pvw_shamir_erasure_mask_device(ctx: *mut PvwCtx, d_status: *mut u32, d_noise: *const u64, status_bits: u32, noise_bound: u64, count: usize, num_secrets: usize, secret_stride: usize, point_stride: usize, d_mask_out: *mut u64, stream: *mut c_void) -> i32;
    // ---- decrypt (src/crypto/decryption.rs:249-325) and gadget decode (:10-247) ---------------
    pub fn pvw_decrypt_batch(ctx: *mut PvwCtx, sk: *const i64, c1s: *const u64, c2col: *const u64, num_dealers: usize, in_repr: u32, out_u64: *mut u64, noisy_out: *mut u64) -> i32;
    pub fn pvw_decrypt_noisy_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_batch_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_sk_load(ctx: *mut PvwCtx, sk: *const i64, out: *mut *mut PvwSk) -> i32;
    pub fn pvw_sk_load_seeded(ctx: *mut PvwCtx, sk_seed: *const u8, party_index: u32, out: *mut *mut PvwSk) -> i32;
    pub fn pvw_sk_free(key: *mut PvwSk) -> i32;
    pub fn pvw_decrypt_batch_device_sk(ctx: *mut PvwCtx, key: *const PvwSk, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, in_repr: u32, out_u64: *mut u64) -> i32;
    pub fn pvw_decrypt_all_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, in_repr: u32, d_out: *mut u64, stream: *mut c_void) -> i32;
    // ---- checked decryption: noise / status per share -------------------------------
    pub fn pvw_decrypt_batch_checked(ctx: *mut PvwCtx, sk: *const i64, c1s: *const u64, c2col: *const u64, num_dealers: usize, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32) -> i32;
    pub fn pvw_decrypt_batch_checked_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_batch_device_sk_checked(ctx: *mut PvwCtx, key: *const PvwSk, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_checked(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32) -> i32;
    pub fn pvw_decrypt_all_checked_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decode_checked(ctx: *mut PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, noise: *mut u64, status: *mut u32) -> i32;
    pub fn pvw_decode_checked_device(ctx: *mut PvwCtx, d_noisy: *const u64, count: usize, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decode_checked_host(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, noise: *mut u64, status: *mut u32) -> i32;
    pub fn pvw_selftest_decode_checked(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, noise: *mut u64, status: *mut u32) -> i32;
    pub fn pvw_ctx_noise_bound(ctx: *const PvwCtx, out: *mut u64) -> i32;
    pub fn pvw_ct_sum_device(ctx: *mut PvwCtx, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, row_lo: u32, row_hi: u32, d_c1_out: *mut u64, d_c2_out: *mut u64, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_ct_sum(ctx: *mut PvwCtx, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, row_lo: u32, row_hi: u32, c1_out: *mut u64, c2_out: *mut u64, count: *mut u32) -> i32;
    pub fn pvw_ct_sum_host(ctx: *const PvwCtx, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, row_lo: u32, row_hi: u32, c1_out: *mut u64, c2_out: *mut u64, count: *mut u32) -> i32;
    pub fn pvw_decrypt_sum_checked_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, d_valid: *const u8, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_sum_device_sk_checked(ctx: *mut PvwCtx, key: *const PvwSk, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, d_valid: *const u8, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_sum_checked(ctx: *mut PvwCtx, sk: *const i64, c1s: *const u64, c2col: *const u64, num_dealers: usize, valid: *const u8, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32) -> i32;
    pub fn pvw_decrypt_all_sum_checked(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32) -> i32;
    pub fn pvw_decrypt_all_sum_checked_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_ctx_sum_capacity(ctx: *const PvwCtx, max_dealers: *mut u64) -> i32;
    // ---- plain-modulus decode: the checked call plus (plain_modulus, wide_words, wide) ----
    pub fn pvw_decode_plain(ctx: *mut PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, noise: *mut u64, status: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decode_plain_device(ctx: *mut PvwCtx, d_noisy: *const u64, count: usize, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decode_plain_host(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, noise: *mut u64, status: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_selftest_decode_plain(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, noise: *mut u64, status: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_batch_plain(ctx: *mut PvwCtx, sk: *const i64, c1s: *const u64, c2col: *const u64, num_dealers: usize, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_batch_plain_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_batch_device_sk_plain(ctx: *mut PvwCtx, key: *const PvwSk, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_plain(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_all_plain_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_sum_plain(ctx: *mut PvwCtx, sk: *const i64, c1s: *const u64, c2col: *const u64, num_dealers: usize, valid: *const u8, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_sum_plain_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, d_valid: *const u8, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_sum_device_sk_plain(ctx: *mut PvwCtx, key: *const PvwSk, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, d_valid: *const u8, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_sum_plain(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_all_sum_plain_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    // ---- weighted sums of dealers' ciphertexts: the sum calls plus `weights` directly after `valid` ----
    pub fn pvw_ct_lincomb_device(ctx: *mut PvwCtx, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, d_weights: *const i64, row_lo: u32, row_hi: u32, d_c1_out: *mut u64, d_c2_out: *mut u64, d_count: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_ct_lincomb(ctx: *mut PvwCtx, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, row_lo: u32, row_hi: u32, c1_out: *mut u64, c2_out: *mut u64, count: *mut u32) -> i32;
    pub fn pvw_ct_lincomb_host(ctx: *const PvwCtx, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, row_lo: u32, row_hi: u32, c1_out: *mut u64, c2_out: *mut u64, count: *mut u32) -> i32;
    pub fn pvw_decrypt_lincomb_plain(ctx: *mut PvwCtx, sk: *const i64, c1s: *const u64, c2col: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_lincomb_plain_device(ctx: *mut PvwCtx, d_sk: *const i64, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, d_valid: *const u8, d_weights: *const i64, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_lincomb_device_sk_plain(ctx: *mut PvwCtx, key: *const PvwSk, d_c1s: *const u64, d_c2col: *const u64, num_dealers: usize, d_valid: *const u8, d_weights: *const i64, in_repr: u32, d_noisy: *mut u64, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_lincomb_plain(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, count: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decrypt_all_lincomb_plain_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, d_weights: *const i64, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_count: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_ctx_lincomb_fits(ctx: *const PvwCtx, weights: *const i64, num_dealers: usize, valid: *const u8, fits: *mut u32) -> i32;
    pub fn pvw_shamir_lagrange_weights(plain_modulus: u64, indices: *const u64, count: usize, weights_out: *mut i64) -> i32;
    // many combinations of the same dealers' ciphertexts
    pub fn pvw_shamir_lagrange_weights_at(plain_modulus: u64, indices: *const u64, count: usize, targets: *const u64, num_targets: usize, weights_out: *mut i64) -> i32;
    pub fn pvw_ct_lincomb_many_host(ctx: *const PvwCtx, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, num_combos: usize, row_lo: u32, row_hi: u32, c1_out: *mut u64, c2_out: *mut u64, counts: *mut u32) -> i32;
    pub fn pvw_ct_lincomb_many_device(ctx: *mut PvwCtx, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, d_weights: *const i64, num_combos: usize, row_lo: u32, row_hi: u32, d_c1_out: *mut u64, d_c2_out: *mut u64, d_counts: *mut u32, stream: *mut c_void) -> i32;
    pub fn pvw_ct_lincomb_many(ctx: *mut PvwCtx, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, num_combos: usize, row_lo: u32, row_hi: u32, c1_out: *mut u64, c2_out: *mut u64, counts: *mut u32) -> i32;
    pub fn pvw_decrypt_all_lincomb_many_plain_device(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, d_sk: *const i64, d_c1s: *const u64, d_c2s: *const u64, num_dealers: usize, d_valid: *const u8, d_weights: *const i64, num_combos: usize, in_repr: u32, d_out: *mut u64, d_noise: *mut u64, d_status: *mut u32, d_counts: *mut u32, plain_modulus: u64, wide_words: u32, d_wide: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_decrypt_all_lincomb_many_plain(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, sk: *const i64, c1s: *const u64, c2s: *const u64, num_dealers: usize, valid: *const u8, weights: *const i64, num_combos: usize, in_repr: u32, out_u64: *mut u64, noise: *mut u64, status: *mut u32, counts: *mut u32, plain_modulus: u64, wide_words: u32, wide: *mut u64) -> i32;
    pub fn pvw_decode(ctx: *mut PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64) -> i32;
    pub fn pvw_decode_host(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64) -> i32;
    pub fn pvw_decode_device(ctx: *mut PvwCtx, d_noisy: *const u64, count: usize, d_out: *mut u64, stream: *mut c_void) -> i32;
    // ---- self-tests / build identity -------------------------------------------------------------
    pub fn pvw_selftest_decode_fixed(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64) -> i32;
    pub fn pvw_selftest_mfma_i8(ctx: *mut PvwCtx, a: *const i8, b: *const i8, out: *mut i32) -> i32;
    pub fn pvw_selftest_secret_residue(ctx: *mut PvwCtx, nonzero_words: *mut u64, scanned_words: *mut u64) -> i32;
    pub fn pvw_selftest_siphash(msg: *const u8, len: usize, k0: u64, k1: u64, c_rounds: i32, d_rounds: i32, out: *mut u64) -> i32;
    pub fn pvw_selftest_decode_tables(ctx: *const PvwCtx, info_out: *mut u32) -> i32;
    pub fn pvw_selftest_decode_shortcuts(ctx: *const PvwCtx, noisy: *const u64, count: usize, out_u64: *mut u64, short_path: *mut u8) -> i32;
    pub fn pvw_selftest_rnd_free_residue(nonzero_words: *mut u64) -> i32;
    pub fn pvw_build_is_tuning() -> i32;
    // ---- ring primitives (fhe-math call sites: change_representation, from_coefficients) ---------
    pub fn pvw_ntt_forward(ctx: *mut PvwCtx, polys: *mut u64, count: usize) -> i32;
    pub fn pvw_ntt_inverse(ctx: *mut PvwCtx, polys: *mut u64, count: usize) -> i32;
    pub fn pvw_small_to_poly(ctx: *mut PvwCtx, coeffs: *const i64, count: usize, polys: *mut u64, repr: u32) -> i32;
    // ---- samplers (src/sampling/uniform.rs:5-70, normal.rs:12-20,136-190) ------------------------
    pub fn pvw_sample_cbd(ctx: *mut PvwCtx, seed: *const u8, domain: u32, index0: u32, count: usize, variance: f32, out: *mut i64) -> i32;
    pub fn pvw_sample_uniform(ctx: *mut PvwCtx, seed: *const u8, domain: u32, index0: u32, count: usize, bound: u64, out: *mut i64) -> i32;
    pub fn pvw_sample_gaussian(ctx: *mut PvwCtx, seed: *const u8, index0: u32, count: usize, bound: u64, out: *mut i64) -> i32;
    // ---- measurement hooks -----------------------------------------------------------------------
    pub fn pvw_ctx_set_profiling(ctx: *mut PvwCtx, on: i32) -> i32;
    pub fn pvw_ctx_kernel_time(ctx: *mut PvwCtx, name: *const c_char, total_ms: *mut f64, launches: *mut u64) -> i32;
    pub fn pvw_ctx_reset_profiling(ctx: *mut PvwCtx) -> i32;
    pub fn pvw_host_alloc(bytes: usize, out: *mut *mut c_void) -> i32;
    pub fn pvw_host_free(p: *mut c_void) -> i32;
    pub fn pvw_ctx_resident_bytes(ctx: *const PvwCtx, crs_bytes: *mut u64, pk_bytes: *mut u64) -> i32;
    pub fn pvw_ctx_derived_bytes(ctx: *const PvwCtx, packed_bytes: *mut u64, mfma_tiled_bytes: *mut u64) -> i32;
    pub fn pvw_prepare(ctx: *mut PvwCtx, flags: u32, stream: *mut c_void, bytes_out: *mut u64) -> i32;
    pub fn pvw_ctx_packed_active(ctx: *const PvwCtx, width_out: *mut u32) -> i32;
    pub fn pvw_ctx_synchronize(ctx: *mut PvwCtx) -> i32;
    // ---- wire format, version 1; the `pvw` shim keeps fhe-math serde ------------------
    pub fn pvw_wire_poly_bytes(ctx: *const PvwCtx, out: *mut usize) -> i32;
    pub fn pvw_wire_header(ctx: *const PvwCtx, kind: u32, repr: u32, lo: u32, hi: u32, lo2: u32, hi2: u32, out: *mut u8, cap: usize, len: *mut usize) -> i32;
    pub fn pvw_wire_header_check(ctx: *const PvwCtx, data: *const u8, len: usize, kind: *mut u32, repr: *mut u32, ranges: *mut u32, header_len: *mut usize) -> i32;
    pub fn pvw_wire_pack(ctx: *mut PvwCtx, polys: *const u64, count: usize, out: *mut u8) -> i32;
    pub fn pvw_wire_pack_device(ctx: *mut PvwCtx, d_polys: *const u64, count: usize, d_out: *mut u8, stream: *mut c_void) -> i32;
    pub fn pvw_wire_unpack(ctx: *mut PvwCtx, data: *const u8, count: usize, polys: *mut u64) -> i32;
    pub fn pvw_wire_unpack_device(ctx: *mut PvwCtx, d_in: *const u8, count: usize, d_polys: *mut u64, d_bad: *mut u64, stream: *mut c_void) -> i32;
    pub fn pvw_wire_pack_host(ctx: *const PvwCtx, polys: *const u64, count: usize, out: *mut u8) -> i32;
    pub fn pvw_wire_unpack_host(ctx: *const PvwCtx, data: *const u8, count: usize, polys: *mut u64, bad_out: *mut u64) -> i32;
    pub fn pvw_load_pk_wire(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, body: *const u8, repr: u32) -> i32;
    pub fn pvw_get_pk_wire(ctx: *mut PvwCtx, party_lo: u32, party_hi: u32, body_out: *mut u8, repr: u32) -> i32;
    pub fn pvw_load_crs_wire(ctx: *mut PvwCtx, body: *const u8, repr: u32) -> i32;
    pub fn pvw_get_crs_wire(ctx: *mut PvwCtx, body_out: *mut u8, repr: u32) -> i32;
}

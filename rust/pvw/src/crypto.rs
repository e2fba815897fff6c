//! `encrypt` / `decrypt_*` over `libpvw_hip.so` (NOT COMPILED here -- see rust/README.md).
//! Replaces the bodies of `src/crypto/encryption.rs:105-296` and `src/crypto/decryption.rs:249-325`; names,
//! signatures, validation order and messages are the reference's.
use std::sync::Arc;

use fhe_math::rq::Poly;
use pvw_hip_sys as sys;
use rand::RngCore;
use zeroize::Zeroize;

use crate::crypto::encryption::PvwCiphertext;
use crate::errors::PvwError;
use crate::ffi_support::{check, poly_from_flat, poly_to_flat, poly_words};
use crate::keys::public_key::GlobalPublicKey;
use crate::keys::secret_key::SecretKey;
use crate::params::{PvwParameters, Result};

fn fresh_seed() -> [u8; 32] {
    let mut seed = [0u8; 32];
    rand::thread_rng().fill_bytes(&mut seed); // fresh randomness per call, as the reference's thread_rng() draws
    seed
}

fn ciphertext_from_flat(c1: &[u64], c2: &[u64], params: &Arc<PvwParameters>) -> Result<PvwCiphertext> {
    let words = poly_words(params);
    let c1: Result<Vec<Poly>> = c1.chunks_exact(words).map(|c| poly_from_flat(c, params)).collect();
    let c2: Result<Vec<Poly>> = c2.chunks_exact(words).map(|c| poly_from_flat(c, params)).collect();
    let ct = PvwCiphertext { c1: c1?, c2: c2?, params: params.clone() };
    ct.validate()?; // encryption.rs:204-211
    Ok(ct)
}

/// `encrypt` (encryption.rs:105-214).  The checks at :109 (scalar count), :117 (key fullness) and :124
/// (correctness condition) run inside `pvw_encrypt` with the reference's messages.
pub fn encrypt(scalars: &[u64], global_pk: &GlobalPublicKey) -> Result<PvwCiphertext> {
    let params = &global_pk.params;
    let words = poly_words(params);
    let rnd = sys::PvwRandomnessT {
        mode: sys::PVW_RND_SEED,
        seed: fresh_seed(),
        r: std::ptr::null(),
        e1: std::ptr::null(),
        e2: std::ptr::null(),
    };
    let (mut c1, mut c2) = (vec![0u64; params.k * words], vec![0u64; params.n * words]);
    check(unsafe {
        sys::pvw_encrypt(params.hip.raw(), scalars.as_ptr(), scalars.len(), &rnd, c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    ciphertext_from_flat(&c1, &c2, params)
}

/// A randomness state on the device (`pvw_rnd_state`): a seed drawn ONCE from `thread_rng` and a counter.  `encrypt_with` /
/// `encrypt_all_party_shares_with` draw call `i`'s randomness from it on the device (`call_seed(S, c + i)`) and advance the
/// counter there, so no host work per call is needed for fresh randomness, and device-pointer calls captured into a graph
/// draw anew on every replay -- the reference's contract (`thread_rng()` on every encrypt, encryption.rs:135-167).
/// Holds its parameters, so the context it was created for outlives it; dropping it clears the device seed.
pub struct DeviceRandomness {
    params: Arc<PvwParameters>,
    raw: *mut std::ffi::c_void,
}

impl DeviceRandomness {
    pub fn new(params: &Arc<PvwParameters>) -> Result<Self> {
        let mut seed = fresh_seed();
        let mut raw: *mut std::ffi::c_void = std::ptr::null_mut();
        let rc = unsafe { sys::pvw_rnd_state_create(params.hip.raw(), seed.as_ptr(), 0, &mut raw) };
        seed.zeroize();
        check(rc)?;
        Ok(Self { params: params.clone(), raw })
    }

    /// the counter once the work on the context's stream is done
    pub fn counter(&self) -> Result<u64> {
        let mut v = 0u64;
        check(unsafe { sys::pvw_rnd_state_counter(self.raw, std::ptr::null_mut(), &mut v) })?;
        Ok(v)
    }

    pub fn params(&self) -> &Arc<PvwParameters> {
        &self.params
    }

    pub fn raw(&self) -> *mut std::ffi::c_void {
        self.raw
    }
}

impl Drop for DeviceRandomness {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            unsafe { sys::pvw_rnd_state_free(self.raw) };
            self.raw = std::ptr::null_mut();
        }
    }
}

/// `encrypt` with the randomness drawn from a `DeviceRandomness` on the device.
pub fn encrypt_with(scalars: &[u64], global_pk: &GlobalPublicKey, rnd: &DeviceRandomness) -> Result<PvwCiphertext> {
    let params = &global_pk.params;
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; params.k * words], vec![0u64; params.n * words]);
    check(unsafe {
        sys::pvw_encrypt_rs(params.hip.raw(), scalars.as_ptr(), scalars.len(), rnd.raw(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    ciphertext_from_flat(&c1, &c2, params)
}

/// `encrypt_party_shares` (encryption.rs:221-245).
pub fn encrypt_party_shares(party_shares: &[u64], party_index: usize, global_pk: &GlobalPublicKey) -> Result<PvwCiphertext> {
    if party_index >= global_pk.params.n {
        return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party_index, global_pk.params.n - 1)));
    }
    if party_shares.len() != global_pk.params.n {
        return Err(PvwError::InvalidParameters(format!("Party must provide {} shares, got {}", global_pk.params.n, party_shares.len())));
    }
    encrypt(party_shares, global_pk)
}

/// `encrypt_all_party_shares` (encryption.rs:253-286): ONE device call for all dealers instead of a rayon loop
/// over `encrypt` -- the dealers share passes over the resident public key (matrix cores from 3 dealers up), each
/// with its own seed.
pub fn encrypt_all_party_shares(all_shares: &[Vec<u64>], global_pk: &GlobalPublicKey) -> Result<Vec<PvwCiphertext>> {
    let params = &global_pk.params;
    let n = params.n;
    if all_shares.len() != n {
        return Err(PvwError::InvalidParameters(format!("Must provide shares for all {n} parties")));
    }
    for (dealer_idx, dealer_shares) in all_shares.iter().enumerate() {
        if dealer_shares.len() != n {
            return Err(PvwError::InvalidParameters(format!(
                "Dealer {} provided {} shares but needs {}",
                dealer_idx,
                dealer_shares.len(),
                n
            )));
        }
    }
    let words = poly_words(params);
    let scalars: Vec<u64> = all_shares.iter().flat_map(|row| row.iter().copied()).collect();
    let mut seeds = vec![0u8; 32 * n];
    rand::thread_rng().fill_bytes(&mut seeds);
    let (mut c1, mut c2) = (vec![0u64; n * params.k * words], vec![0u64; n * n * words]);
    check(unsafe {
        sys::pvw_encrypt_multi(params.hip.raw(), scalars.as_ptr(), n, n, seeds.as_ptr(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    (0..n)
        .map(|d| ciphertext_from_flat(&c1[d * params.k * words..(d + 1) * params.k * words], &c2[d * n * words..(d + 1) * n * words], params))
        .collect()
}

/// `encrypt_all_party_shares` with dealer d's randomness drawn from a `DeviceRandomness` (`call_seed(S, c + d)`).
pub fn encrypt_all_party_shares_with(all_shares: &[Vec<u64>], global_pk: &GlobalPublicKey, rnd: &DeviceRandomness) -> Result<Vec<PvwCiphertext>> {
    let params = &global_pk.params;
    let n = params.n;
    if all_shares.len() != n {
        return Err(PvwError::InvalidParameters(format!("Must provide shares for all {n} parties")));
    }
    for (dealer_idx, dealer_shares) in all_shares.iter().enumerate() {
        if dealer_shares.len() != n {
            return Err(PvwError::InvalidParameters(format!(
                "Dealer {} provided {} shares but needs {}",
                dealer_idx,
                dealer_shares.len(),
                n
            )));
        }
    }
    let words = poly_words(params);
    let scalars: Vec<u64> = all_shares.iter().flat_map(|row| row.iter().copied()).collect();
    let (mut c1, mut c2) = (vec![0u64; n * params.k * words], vec![0u64; n * n * words]);
    check(unsafe {
        sys::pvw_encrypt_multi_rs(params.hip.raw(), scalars.as_ptr(), n, n, rnd.raw(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    (0..n)
        .map(|d| ciphertext_from_flat(&c1[d * params.k * words..(d + 1) * params.k * words], &c2[d * n * words..(d + 1) * n * words], params))
        .collect()
}

/// `encrypt_broadcast` (encryption.rs:292-296).
pub fn encrypt_broadcast(scalar: u64, global_pk: &GlobalPublicKey) -> Result<PvwCiphertext> {
    let broadcast_values = vec![scalar; global_pk.params.n];
    encrypt(&broadcast_values, global_pk)
}

fn flat_secret(sk: &SecretKey) -> Vec<i64> {
    sk.secret_coeffs.iter().flat_map(|row| row.iter().copied()).collect()
}

/// A `SecretKey` kept on the device in the form the inner products of decrypt read (`pvw_sk_load`: NTT(sk[j]), what
/// `SecretKey::get_polynomial` computes k times per `decrypt_party_value`, secret_key.rs:98-112 / decryption.rs:260).  For a
/// receiver that decrypts many device-resident ciphertext batches under one key: `pvw_decrypt_batch_device_sk` then neither
/// transforms nor wipes per call.  Dropping the handle clears the device copy (`pvw_sk_free`), as dropping the reference's
/// `SecretKey` zeroizes it (secret_key.rs:20-30).  Must not outlive the `PvwParameters` it was loaded for.
pub struct DeviceSecretKey {
    raw: *mut sys::PvwSk,
}

impl DeviceSecretKey {
    pub fn load(secret_key: &SecretKey) -> Result<Self> {
        let mut sk = flat_secret(secret_key);
        let mut raw: *mut sys::PvwSk = std::ptr::null_mut();
        let rc = unsafe { sys::pvw_sk_load(secret_key.params.hip.raw(), sk.as_ptr(), &mut raw) };
        sk.zeroize();
        check(rc)?;
        Ok(Self { raw })
    }

    pub fn raw(&self) -> *const sys::PvwSk {
        self.raw
    }
}

impl Drop for DeviceSecretKey {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            unsafe { sys::pvw_sk_free(self.raw) };
            self.raw = std::ptr::null_mut();
        }
    }
}

/// `decrypt_party_value` (decryption.rs:249-278): <sk, c1> - c2[party_index], inverse NTT and the gadget decode
/// (`decode_scalar_pvw_rns`, :10-58) all on the device; one u64 comes back.
pub fn decrypt_party_value(ciphertext: &PvwCiphertext, secret_key: &SecretKey, party_index: usize) -> Result<u64> {
    let params = &ciphertext.params;
    let mut c1s = Vec::with_capacity(params.k * poly_words(params));
    for poly in ciphertext.c1.iter() {
        poly_to_flat(poly, &mut c1s);
    }
    let mut c2col = Vec::with_capacity(poly_words(params));
    poly_to_flat(&ciphertext.c2[party_index], &mut c2col);
    let mut sk = flat_secret(secret_key);
    let mut out = 0u64;
    let rc = unsafe {
        sys::pvw_decrypt_batch(params.hip.raw(), sk.as_ptr(), c1s.as_ptr(), c2col.as_ptr(), 1, sys::PVW_REPR_POWER, &mut out, std::ptr::null_mut())
    };
    sk.zeroize();
    check(rc)?;
    Ok(out)
}

/// `decrypt_party_shares` (decryption.rs:281-325): one batched device pass over all dealers' ciphertexts.
pub fn decrypt_party_shares(all_ciphertexts: &[PvwCiphertext], secret_key: &SecretKey, party_index: usize) -> Result<Vec<u64>> {
    if all_ciphertexts.is_empty() {
        return Err(PvwError::InvalidParameters("No ciphertexts provided".to_string()));
    }
    let params = &all_ciphertexts[0].params;
    if all_ciphertexts.len() != params.n {
        return Err(PvwError::InvalidParameters(format!("Expected {} ciphertexts, got {}", params.n, all_ciphertexts.len())));
    }
    if party_index >= params.n {
        return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party_index, params.n - 1)));
    }
    let words = poly_words(params);
    let d = all_ciphertexts.len();
    let (mut c1s, mut c2col) = (Vec::with_capacity(d * params.k * words), Vec::with_capacity(d * words));
    for (dealer_idx, ciphertext) in all_ciphertexts.iter().enumerate() {
        ciphertext
            .validate()
            .map_err(|e| PvwError::InvalidParameters(format!("Ciphertext {dealer_idx} invalid: {e}")))?;
        for poly in ciphertext.c1.iter() {
            poly_to_flat(poly, &mut c1s);
        }
        poly_to_flat(&ciphertext.c2[party_index], &mut c2col);
    }
    let mut sk = flat_secret(secret_key);
    let mut out = vec![0u64; d];
    let rc = unsafe {
        sys::pvw_decrypt_batch(params.hip.raw(), sk.as_ptr(), c1s.as_ptr(), c2col.as_ptr(), d, sys::PVW_REPR_POWER, out.as_mut_ptr(), std::ptr::null_mut())
    };
    sk.zeroize();
    check(rc)?;
    Ok(out)
}

/// EXTENSION: `decrypt_party_shares` with each share's report (`pvw_decrypt_batch_checked`) -- the same checks
/// and values, plus `noise[d]` (max |residual|, saturating at u64::MAX) and `lossy[d]` (the value is not the plaintext).
/// A share is valid when it is not lossy and its noise is at most the caller's bound (e.g. `pvw_ctx_noise_bound`).
pub fn decrypt_party_shares_checked(all_ciphertexts: &[PvwCiphertext], secret_key: &SecretKey, party_index: usize) -> Result<(Vec<u64>, Vec<u64>, Vec<bool>)> {
    let r = decrypt_party_shares_plain(all_ciphertexts, secret_key, party_index, &PlainOptions::default())?;
    Ok((r.values, r.noise, r.status.iter().map(|s| s & sys::PVW_DEC_LOSSY != 0).collect()))
}

/// EXTENSION: the plain options of a decrypt.  `modulus` 0 = none, else 2 <= modulus < 2^62 (any integer): the
/// values come back as P mod modulus, the mathematical residue, where the u64 conversion of decryption.rs:226-247 returns 0
/// for P < 0 or P >= 2^64.  `wide_words` 0 = none, else 1 ..= words of Q: the low words of |P| per share.  Both 0: the
/// checked call as it is.
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct PlainOptions {
    pub modulus: u64,
    pub wide_words: u32,
}

/// What a plain decrypt reports: per share the value, the noise, the status bits (`PVW_DEC_LOSSY`,
/// `PVW_DEC_NEGATIVE`, `PVW_DEC_WIDE_TRUNCATED`) and `wide_words` little-endian words of |P| (empty when none were asked for).
#[derive(Clone, Debug, Default)]
pub struct PlainDecryption {
    pub values: Vec<u64>,
    pub noise: Vec<u64>,
    pub status: Vec<u32>,
    pub wide: Vec<u64>,
}

fn wide_ptr(wide: &mut Vec<u64>) -> *mut u64 {
    if wide.is_empty() { std::ptr::null_mut() } else { wide.as_mut_ptr() }
}

/// EXTENSION: `decrypt_party_shares_checked` with the plain options (`pvw_decrypt_batch_plain`).
pub fn decrypt_party_shares_plain(all_ciphertexts: &[PvwCiphertext], secret_key: &SecretKey, party_index: usize, plain: &PlainOptions) -> Result<PlainDecryption> {
    if all_ciphertexts.is_empty() {
        return Err(PvwError::InvalidParameters("No ciphertexts provided".to_string()));
    }
    let params = &all_ciphertexts[0].params;
    if all_ciphertexts.len() != params.n {
        return Err(PvwError::InvalidParameters(format!("Expected {} ciphertexts, got {}", params.n, all_ciphertexts.len())));
    }
    if party_index >= params.n {
        return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party_index, params.n - 1)));
    }
    let words = poly_words(params);
    let d = all_ciphertexts.len();
    let (mut c1s, mut c2col) = (Vec::with_capacity(d * params.k * words), Vec::with_capacity(d * words));
    for (dealer_idx, ciphertext) in all_ciphertexts.iter().enumerate() {
        ciphertext
            .validate()
            .map_err(|e| PvwError::InvalidParameters(format!("Ciphertext {dealer_idx} invalid: {e}")))?;
        for poly in ciphertext.c1.iter() {
            poly_to_flat(poly, &mut c1s);
        }
        poly_to_flat(&ciphertext.c2[party_index], &mut c2col);
    }
    let mut sk = flat_secret(secret_key);
    let (mut out, mut noise, mut status) = (vec![0u64; d], vec![0u64; d], vec![0u32; d]);
    let mut wide = vec![0u64; d * plain.wide_words as usize];
    let rc = unsafe {
        sys::pvw_decrypt_batch_plain(params.hip.raw(), sk.as_ptr(), c1s.as_ptr(), c2col.as_ptr(), d, sys::PVW_REPR_POWER, out.as_mut_ptr(),
                                     noise.as_mut_ptr(), status.as_mut_ptr(), plain.modulus, plain.wide_words, wide_ptr(&mut wide))
    };
    sk.zeroize();
    check(rc)?;
    Ok(PlainDecryption { values: out, noise, status, wide })
}

/// EXTENSION -- no single reference function behind it.  The loop examples/pvw.rs:138-149 and tests/crypto.rs:284-287
/// run over `decrypt_party_shares` for every party, as one call: `results[recipient][dealer]` (examples/pvw.rs:157-170)
/// from one digit GEMM of the parties' keys against all dealers' c1 (`pvw_decrypt_all`).  `parties` must carry
/// consecutive indices; the checks and messages are those of decryption.rs:286-305, per party.
pub fn decrypt_all_party_shares(all_ciphertexts: &[PvwCiphertext], parties: &[crate::keys::public_key::Party]) -> Result<Vec<Vec<u64>>> {
    if all_ciphertexts.is_empty() {
        return Err(PvwError::InvalidParameters("No ciphertexts provided".to_string()));
    }
    let params = &all_ciphertexts[0].params;
    if all_ciphertexts.len() != params.n {
        return Err(PvwError::InvalidParameters(format!("Expected {} ciphertexts, got {}", params.n, all_ciphertexts.len())));
    }
    if parties.is_empty() {
        return Ok(Vec::new());
    }
    let lo = parties[0].index;
    for (i, party) in parties.iter().enumerate() {
        if party.index >= params.n {
            return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party.index, params.n - 1)));
        }
        if party.index != lo + i {
            return Err(PvwError::InvalidParameters(format!("Party indices must be consecutive: {} follows {}", party.index, lo + i - 1)));
        }
    }
    let words = poly_words(params);
    let d = all_ciphertexts.len();
    let (mut c1s, mut c2s) = (Vec::with_capacity(d * params.k * words), Vec::with_capacity(d * params.n * words));
    for (dealer_idx, ciphertext) in all_ciphertexts.iter().enumerate() {
        ciphertext
            .validate()
            .map_err(|e| PvwError::InvalidParameters(format!("Ciphertext {dealer_idx} invalid: {e}")))?;
        for poly in ciphertext.c1.iter() {
            poly_to_flat(poly, &mut c1s);
        }
        for poly in ciphertext.c2.iter() {
            poly_to_flat(poly, &mut c2s);
        }
    }
    let mut sk: Vec<i64> = parties.iter().flat_map(|p| flat_secret(&p.secret_key)).collect();
    let np = parties.len();
    let mut out = vec![0u64; np * d];
    let rc = unsafe {
        sys::pvw_decrypt_all(params.hip.raw(), lo as u32, (lo + np) as u32, sk.as_ptr(), c1s.as_ptr(), c2s.as_ptr(), d, sys::PVW_REPR_POWER, out.as_mut_ptr())
    };
    sk.zeroize();
    check(rc)?;
    Ok(out.chunks_exact(d).map(|r| r.to_vec()).collect())
}

/// The checks and flat buffers every sum shares: (c1s, c2s, valid bytes or empty = every dealer).
fn sum_inputs(ciphertexts: &[PvwCiphertext], valid: Option<&[bool]>) -> Result<(Vec<u64>, Vec<u64>, Vec<u8>)> {
    if ciphertexts.is_empty() {
        return Err(PvwError::InvalidParameters("No ciphertexts provided".to_string()));
    }
    let params = &ciphertexts[0].params;
    if let Some(v) = valid {
        if v.len() != ciphertexts.len() {
            return Err(PvwError::DimensionMismatch { expected: ciphertexts.len(), actual: v.len() });
        }
        if !v.iter().any(|&b| b) {
            return Err(PvwError::InsufficientData { expected: 1, actual: 0 });
        }
    }
    let words = poly_words(params);
    let d = ciphertexts.len();
    let (mut c1s, mut c2s) = (Vec::with_capacity(d * params.k * words), Vec::with_capacity(d * params.n * words));
    for (dealer_idx, ciphertext) in ciphertexts.iter().enumerate() {
        ciphertext
            .validate()
            .map_err(|e| PvwError::InvalidParameters(format!("Ciphertext {dealer_idx} invalid: {e}")))?;
        for poly in ciphertext.c1.iter() {
            poly_to_flat(poly, &mut c1s);
        }
        for poly in ciphertext.c2.iter() {
            poly_to_flat(poly, &mut c2s);
        }
    }
    Ok((c1s, c2s, valid.map(|v| v.iter().map(|&b| b as u8).collect()).unwrap_or_default()))
}

fn valid_ptr(valid: &[u8]) -> *const u8 {
    if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() }
}

/// EXTENSION: dealer d shares `secrets[d]` among the n parties with a random polynomial of `degree` over
/// Z_`plain_modulus` (prime, n < p < 2^62) and encrypts the shares, in ONE device call (`pvw_deal_shares`): neither the
/// shares nor the coefficients exist on the host.  Each dealer's seed comes from `thread_rng` and is cleared afterwards.
pub fn deal_party_shares(secrets: &[u64], degree: u32, plain_modulus: u64, global_pk: &GlobalPublicKey) -> Result<Vec<PvwCiphertext>> {
    let params = &global_pk.params;
    let (n, dealers) = (params.n, secrets.len());
    let words = poly_words(params);
    let mut seeds = vec![0u8; 32 * dealers];
    rand::thread_rng().fill_bytes(&mut seeds);
    let (mut c1, mut c2) = (vec![0u64; dealers * params.k * words], vec![0u64; dealers * n * words]);
    let rc = unsafe {
        sys::pvw_deal_shares(params.hip.raw(), secrets.as_ptr(), dealers, degree, plain_modulus, seeds.as_ptr(), c1.as_mut_ptr(), c2.as_mut_ptr(),
                             sys::PVW_REPR_POWER)
    };
    seeds.zeroize();
    check(rc)?;
    (0..dealers)
        .map(|d| ciphertext_from_flat(&c1[d * params.k * words..(d + 1) * params.k * words], &c2[d * n * words..(d + 1) * n * words], params))
        .collect()
}

/// `deal_party_shares` with dealer d's randomness drawn from a `DeviceRandomness` (`call_seed(S, c + d)`).
pub fn deal_party_shares_with(secrets: &[u64], degree: u32, plain_modulus: u64, global_pk: &GlobalPublicKey, rnd: &DeviceRandomness) -> Result<Vec<PvwCiphertext>> {
    let params = &global_pk.params;
    let (n, dealers) = (params.n, secrets.len());
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; dealers * params.k * words], vec![0u64; dealers * n * words]);
    check(unsafe {
        sys::pvw_deal_shares_rs(params.hip.raw(), secrets.as_ptr(), dealers, degree, plain_modulus, rnd.raw(), c1.as_mut_ptr(), c2.as_mut_ptr(),
                                sys::PVW_REPR_POWER)
    })?;
    (0..dealers)
        .map(|d| ciphertext_from_flat(&c1[d * params.k * words..(d + 1) * params.k * words], &c2[d * n * words..(d + 1) * n * words], params))
        .collect()
}

/// EXTENSION: packed dealing.  `secrets` is `[dealers][pack]` row-major: dealer d's `pack` secrets sit at the
/// points 0, -1, ..., -(pack-1) of ONE polynomial with `degree` random coefficients, so `pack` secrets cost one ciphertext
/// (`pvw_deal_shares_packed`).  `pack = 1` is `deal_party_shares`.  Seeds as there.
pub fn deal_party_shares_packed(secrets: &[u64], pack: u32, degree: u32, plain_modulus: u64, global_pk: &GlobalPublicKey) -> Result<Vec<PvwCiphertext>> {
    if pack == 0 || secrets.len() % pack as usize != 0 {
        return Err(PvwError::InvalidParameters("secrets must hold pack values per dealer".into()));
    }
    let params = &global_pk.params;
    let (n, dealers) = (params.n, secrets.len() / pack as usize);
    let words = poly_words(params);
    let mut seeds = vec![0u8; 32 * dealers];
    rand::thread_rng().fill_bytes(&mut seeds);
    let (mut c1, mut c2) = (vec![0u64; dealers * params.k * words], vec![0u64; dealers * n * words]);
    let rc = unsafe {
        sys::pvw_deal_shares_packed(params.hip.raw(), secrets.as_ptr(), dealers, pack, degree, plain_modulus, seeds.as_ptr(), c1.as_mut_ptr(),
                                    c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    };
    seeds.zeroize();
    check(rc)?;
    (0..dealers)
        .map(|d| ciphertext_from_flat(&c1[d * params.k * words..(d + 1) * params.k * words], &c2[d * n * words..(d + 1) * n * words], params))
        .collect()
}

/// `deal_party_shares_packed` with dealer d's randomness drawn from a `DeviceRandomness` (`call_seed(S, c + d)`).
pub fn deal_party_shares_packed_with(secrets: &[u64], pack: u32, degree: u32, plain_modulus: u64, global_pk: &GlobalPublicKey,
                                     rnd: &DeviceRandomness) -> Result<Vec<PvwCiphertext>> {
    if pack == 0 || secrets.len() % pack as usize != 0 {
        return Err(PvwError::InvalidParameters("secrets must hold pack values per dealer".into()));
    }
    let params = &global_pk.params;
    let (n, dealers) = (params.n, secrets.len() / pack as usize);
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; dealers * params.k * words], vec![0u64; dealers * n * words]);
    check(unsafe {
        sys::pvw_deal_shares_packed_rs(params.hip.raw(), secrets.as_ptr(), dealers, pack, degree, plain_modulus, rnd.raw(), c1.as_mut_ptr(),
                                       c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    (0..dealers)
        .map(|d| ciphertext_from_flat(&c1[d * params.k * words..(d + 1) * params.k * words], &c2[d * n * words..(d + 1) * n * words], params))
        .collect()
}

/// EXTENSION: the packed shares themselves, `[dealers][n]` row-major (`pvw_shamir_shares_packed`).
pub fn shamir_shares_packed(params: &Arc<PvwParameters>, secrets: &[u64], pack: u32, degree: u32, plain_modulus: u64, seeds: Option<&[u8]>,
                            coeffs: Option<&[u64]>) -> Result<Vec<u64>> {
    if pack == 0 || secrets.len() % pack as usize != 0 {
        return Err(PvwError::InvalidParameters("secrets must hold pack values per dealer".into()));
    }
    let dealers = secrets.len() / pack as usize;
    let mut out = vec![0u64; dealers * params.n];
    check(unsafe {
        sys::pvw_shamir_shares_packed(params.hip.raw(), secrets.as_ptr(), dealers, pack, degree, plain_modulus,
                                      seeds.map_or(std::ptr::null(), |s| s.as_ptr()), coeffs.map_or(std::ptr::null(), |c| c.as_ptr()), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// EXTENSION: the `pack` secrets of every row, `[rows][pack]` row-major, from the shares `[rows][indices.len()]`
/// of the parties `indices` (at least degree + pack of them).  Host only (`pvw_shamir_reconstruct_packed`).
pub fn shamir_reconstruct_packed(indices: &[u64], shares: &[u64], plain_modulus: u64, pack: u32) -> Result<Vec<u64>> {
    if indices.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one value per index and row".into()));
    }
    let rows = shares.len() / indices.len();
    let mut out = vec![0u64; rows * pack as usize];
    check(unsafe { sys::pvw_shamir_reconstruct_packed(plain_modulus, pack, indices.as_ptr(), shares.as_ptr(), indices.len(), rows, out.as_mut_ptr()) })?;
    Ok(out)
}

/// The `targets` of `shamir_evaluate_corrected` that give secrets 1 .. pack-1 of a packed sharing: index p - 1 - j is the point -j.
pub fn shamir_packed_secret_indices(plain_modulus: u64, pack: u32) -> Vec<u64> {
    (1..pack as u64).map(|j| plain_modulus - 1 - j).collect()
}

/// EXTENSION: the secrets of a packed sharing, `[rows][pack]` row-major, although up to
/// `(indices.len() - degree - pack) / 2` shares of each row are wrong: one `shamir_evaluate_corrected` call with polynomial
/// degree `degree + pack - 1`.  Column 0 comes from the call's secrets, the rest from its values; an undecodable row is all 0.
/// `pack = 1` has no targets and is `shamir_reconstruct_corrected`.
pub fn shamir_reconstruct_packed_corrected(params: &Arc<PvwParameters>, indices: &[u64], shares: &[u64], degree: u32, plain_modulus: u64, pack: u32,
                                           party_major: bool) -> Result<(Vec<u64>, CorrectedSecrets)> {
    if pack == 0 {
        return Err(PvwError::InvalidParameters("pack must be at least 1".into()));
    }
    if pack == 1 {
        let r = shamir_reconstruct_corrected(params, indices, shares, degree, plain_modulus, party_major)?;
        return Ok((r.secrets.clone(), r));
    }
    let targets = shamir_packed_secret_indices(plain_modulus, pack);
    let (values, r) = shamir_evaluate_corrected(params, indices, shares, degree + pack - 1, plain_modulus, &targets, party_major)?;
    let k = pack as usize;
    let mut secrets = vec![0u64; r.secrets.len() * k];
    for s in 0..r.secrets.len() {
        secrets[s * k] = r.secrets[s];
        secrets[s * k + 1..(s + 1) * k].copy_from_slice(&values[s * (k - 1)..(s + 1) * (k - 1)]);
    }
    Ok((secrets, r))
}

/// EXTENSION: the shares themselves, `[dealers][n]` row-major, made on the device (`pvw_shamir_shares`) from
/// one 32-byte seed per dealer, or from explicit coefficients `[dealers][degree]`.
pub fn shamir_shares(params: &Arc<PvwParameters>, secrets: &[u64], degree: u32, plain_modulus: u64, seeds: Option<&[u8]>, coeffs: Option<&[u64]>) -> Result<Vec<u64>> {
    let mut out = vec![0u64; secrets.len() * params.n];
    check(unsafe {
        sys::pvw_shamir_shares(params.hip.raw(), secrets.as_ptr(), secrets.len(), degree, plain_modulus,
                               seeds.map_or(std::ptr::null(), |s| s.as_ptr()), coeffs.map_or(std::ptr::null(), |c| c.as_ptr()), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// EXTENSION: the secrets from the shares of the parties `indices` (at least degree + 1 of them):
/// `shares` is `[num_secrets][indices.len()]` row-major.  Host only (`pvw_shamir_reconstruct`).
pub fn shamir_reconstruct(indices: &[u64], shares: &[u64], plain_modulus: u64) -> Result<Vec<u64>> {
    if indices.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one value per index and secret".into()));
    }
    let mut out = vec![0u64; shares.len() / indices.len()];
    check(unsafe { sys::pvw_shamir_reconstruct(plain_modulus, indices.as_ptr(), shares.as_ptr(), indices.len(), out.len(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// EXTENSION: a field element of up to 256 bits, four little-endian words.
pub type Wide = [u64; 4];

/// EXTENSION: the limb ciphertexts per dealer of `deal_party_shares_wide` (`pvw_shamir_wide_limbs`).
pub fn shamir_wide_limbs(plain_modulus: &Wide, limb_bits: u32) -> Result<u32> {
    let mut nl = 0u32;
    check(unsafe { sys::pvw_shamir_wide_limbs(plain_modulus.as_ptr(), limb_bits, &mut nl) })?;
    Ok(nl)
}

/// EXTENSION: the shares `[dealers][n][4]` over an odd prime below 2^256, made on the device
/// (`pvw_shamir_shares_wide`) from one 32-byte seed per dealer or from explicit coefficients `[dealers][degree][4]`.
pub fn shamir_shares_wide(params: &Arc<PvwParameters>, secrets: &[Wide], degree: u32, plain_modulus: &Wide, seeds: Option<&[u8]>, coeffs: Option<&[Wide]>) -> Result<Vec<Wide>> {
    let mut out = vec![[0u64; 4]; secrets.len() * params.n];
    check(unsafe {
        sys::pvw_shamir_shares_wide(params.hip.raw(), secrets.as_ptr() as *const u64, secrets.len(), degree, plain_modulus.as_ptr(),
                                    seeds.map_or(std::ptr::null(), |s| s.as_ptr()), coeffs.map_or(std::ptr::null(), |c| c.as_ptr() as *const u64),
                                    out.as_mut_ptr() as *mut u64)
    })?;
    Ok(out)
}

fn wide_ciphertexts(c1: &[u64], c2: &[u64], vectors: usize, params: &Arc<PvwParameters>) -> Result<Vec<PvwCiphertext>> {
    let (n, words) = (params.n, poly_words(params));
    (0..vectors)
        .map(|v| ciphertext_from_flat(&c1[v * params.k * words..(v + 1) * params.k * words], &c2[v * n * words..(v + 1) * n * words], params))
        .collect()
}

/// EXTENSION: dealer d shares `secrets[d]` over the field of `plain_modulus` and encrypts the shares limb by limb
/// in ONE device call (`pvw_deal_shares_wide`): `dealers * NL` ciphertexts, ciphertext `d * NL + w` carrying limb w of dealer
/// d's shares.  One seed per ciphertext comes from `thread_rng` and is cleared afterwards.
pub fn deal_party_shares_wide(secrets: &[Wide], degree: u32, plain_modulus: &Wide, limb_bits: u32, global_pk: &GlobalPublicKey) -> Result<Vec<PvwCiphertext>> {
    let params = &global_pk.params;
    let vectors = secrets.len() * shamir_wide_limbs(plain_modulus, limb_bits)? as usize;
    let words = poly_words(params);
    let mut seeds = vec![0u8; 32 * vectors];
    rand::thread_rng().fill_bytes(&mut seeds);
    let (mut c1, mut c2) = (vec![0u64; vectors * params.k * words], vec![0u64; vectors * params.n * words]);
    let rc = unsafe {
        sys::pvw_deal_shares_wide(params.hip.raw(), secrets.as_ptr() as *const u64, secrets.len(), degree, plain_modulus.as_ptr(), limb_bits,
                                  seeds.as_ptr(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    };
    seeds.zeroize();
    check(rc)?;
    wide_ciphertexts(&c1, &c2, vectors, params)
}

/// `deal_party_shares_wide` with vector v's randomness drawn from a `DeviceRandomness` (`call_seed(S, c + v)`).
pub fn deal_party_shares_wide_with(secrets: &[Wide], degree: u32, plain_modulus: &Wide, limb_bits: u32, global_pk: &GlobalPublicKey, rnd: &DeviceRandomness) -> Result<Vec<PvwCiphertext>> {
    let params = &global_pk.params;
    let vectors = secrets.len() * shamir_wide_limbs(plain_modulus, limb_bits)? as usize;
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; vectors * params.k * words], vec![0u64; vectors * params.n * words]);
    check(unsafe {
        sys::pvw_deal_shares_wide_rs(params.hip.raw(), secrets.as_ptr() as *const u64, secrets.len(), degree, plain_modulus.as_ptr(), limb_bits,
                                     rnd.raw(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    wide_ciphertexts(&c1, &c2, vectors, params)
}

/// EXTENSION: `values` -> limbs `[num_limbs][values.len()]` (`pvw_shamir_wide_to_limbs_host`).
pub fn shamir_wide_to_limbs(values: &[Wide], limb_bits: u32, num_limbs: u32) -> Result<Vec<u64>> {
    let mut out = vec![0u64; values.len() * num_limbs as usize];
    check(unsafe { sys::pvw_shamir_wide_to_limbs_host(values.as_ptr() as *const u64, values.len(), limb_bits, num_limbs, out.as_mut_ptr()) })?;
    Ok(out)
}

/// EXTENSION: limbs `[num_limbs][count]`, each any word (a limb or a sum of limbs), folded back mod p
/// (`pvw_shamir_wide_from_limbs_host`).
pub fn shamir_wide_from_limbs(plain_modulus: &Wide, limbs: &[u64], limb_bits: u32, num_limbs: u32) -> Result<Vec<Wide>> {
    if num_limbs == 0 || limbs.len() % num_limbs as usize != 0 {
        return Err(PvwError::InvalidParameters("limbs must hold num_limbs rows".into()));
    }
    let count = limbs.len() / num_limbs as usize;
    let mut out = vec![[0u64; 4]; count];
    check(unsafe { sys::pvw_shamir_wide_from_limbs_host(plain_modulus.as_ptr(), limbs.as_ptr(), count, limb_bits, num_limbs, out.as_mut_ptr() as *mut u64) })?;
    Ok(out)
}

/// EXTENSION: the secrets from the shares `[num_secrets][indices.len()]` of the parties `indices` (at least
/// degree + 1 of them).  Host only (`pvw_shamir_reconstruct_wide`).
pub fn shamir_reconstruct_wide(indices: &[u64], shares: &[Wide], plain_modulus: &Wide) -> Result<Vec<Wide>> {
    if indices.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and secret".into()));
    }
    let mut out = vec![[0u64; 4]; shares.len() / indices.len()];
    check(unsafe {
        sys::pvw_shamir_reconstruct_wide(plain_modulus.as_ptr(), indices.as_ptr(), shares.as_ptr() as *const u64, indices.len(), out.len(),
                                         out.as_mut_ptr() as *mut u64)
    })?;
    Ok(out)
}

/// EXTENSION: what `shamir_reconstruct_wide_checked` reports: `CheckedSecrets` with wide secrets.
pub struct CheckedWideSecrets {
    /// the value at 0 of the polynomial through each secret's basis shares
    pub secrets: Vec<Wide>,
    /// per secret: columns beyond the basis whose share is off that polynomial
    pub bad: Vec<u32>,
    /// per column: secrets that deviate there (0 for the basis columns)
    pub col_bad: Vec<u32>,
}

/// EXTENSION: `shamir_reconstruct_checked` over an odd prime below 2^256, on the device
/// (`pvw_shamir_reconstruct_wide_checked`).  The first `degree + 1` of `indices` are the basis.  `shares` is
/// `[num_secrets][indices.len()]` row-major, or with `party_major` `[indices.len()][num_secrets]`; any words, read mod p.
pub fn shamir_reconstruct_wide_checked(params: &Arc<PvwParameters>, indices: &[u64], shares: &[Wide], degree: u32, plain_modulus: &Wide,
                                       party_major: bool) -> Result<CheckedWideSecrets> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and secret".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let mut r = CheckedWideSecrets { secrets: vec![[0u64; 4]; num], bad: vec![0u32; num], col_bad: vec![0u32; count] };
    check(unsafe {
        sys::pvw_shamir_reconstruct_wide_checked(params.hip.raw(), plain_modulus.as_ptr(), degree, indices.as_ptr(), count,
                                                 shares.as_ptr() as *const u64, num, ss, ps, r.secrets.as_mut_ptr() as *mut u64,
                                                 r.bad.as_mut_ptr(), r.col_bad.as_mut_ptr())
    })?;
    Ok(r)
}

/// EXTENSION: what `shamir_reconstruct_wide_corrected` reports: `CorrectedSecrets` with wide secrets.
pub struct CorrectedWideSecrets {
    /// the value at 0 of the one polynomial within E columns of each row; 0 for an undecodable row
    pub secrets: Vec<Wide>,
    /// per secret: columns off that polynomial, or `sys::PVW_SHAMIR_UNDECODABLE`
    pub nerr: Vec<u32>,
    /// per column: decodable secrets that are off there
    pub col_err: Vec<u32>,
    /// `[num_secrets][words]`: bit `c % 64` of word `c / 64` names the columns counted in `nerr`
    pub err_mask: Vec<u64>,
    /// `ceil(indices.len() / 64)`
    pub words: usize,
}

/// EXTENSION: `shamir_reconstruct_corrected` over an odd prime below 2^256, on the device
/// (`pvw_shamir_reconstruct_wide_corrected`): the secrets although up to `(indices.len() - degree - 1) / 2` shares of each are
/// wrong, in whichever columns.  `shares` as `shamir_reconstruct_wide_checked`.
pub fn shamir_reconstruct_wide_corrected(params: &Arc<PvwParameters>, indices: &[u64], shares: &[Wide], degree: u32, plain_modulus: &Wide,
                                         party_major: bool) -> Result<CorrectedWideSecrets> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and secret".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let words = (count + 63) / 64;
    let mut r = CorrectedWideSecrets { secrets: vec![[0u64; 4]; num], nerr: vec![0u32; num], col_err: vec![0u32; count],
                                       err_mask: vec![0u64; num * words], words };
    check(unsafe {
        sys::pvw_shamir_reconstruct_wide_corrected(params.hip.raw(), plain_modulus.as_ptr(), degree, indices.as_ptr(), count,
                                                   shares.as_ptr() as *const u64, num, ss, ps, r.secrets.as_mut_ptr() as *mut u64,
                                                   r.nerr.as_mut_ptr(), r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok(r)
}

/// EXTENSION: `shamir_reconstruct_wide_corrected` with the shares KNOWN to be bad flagged in `erased` (bit `c % 64`
/// of word `c / 64` of row `s`; an earlier call's `err_mask`, or `shamir_wide_erasure_mask`).  Each costs one redundant column
/// instead of two: a row decodes while `2 * errors + erasures <= indices.len() - degree - 1`.  The words at an erased position
/// influence nothing and an erased column is never reported as an error (`pvw_shamir_reconstruct_wide_erasures`).
pub fn shamir_reconstruct_wide_erasures(params: &Arc<PvwParameters>, indices: &[u64], shares: &[Wide], degree: u32, plain_modulus: &Wide,
                                        erased: &[u64], party_major: bool) -> Result<CorrectedWideSecrets> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and secret".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let words = (count + 63) / 64;
    if erased.len() != num * words {
        return Err(PvwError::InvalidParameters("erased must hold ceil(count / 64) words per secret".into()));
    }
    let mut r = CorrectedWideSecrets { secrets: vec![[0u64; 4]; num], nerr: vec![0u32; num], col_err: vec![0u32; count],
                                       err_mask: vec![0u64; num * words], words };
    check(unsafe {
        sys::pvw_shamir_reconstruct_wide_erasures(params.hip.raw(), plain_modulus.as_ptr(), degree, indices.as_ptr(), count,
                                                  shares.as_ptr() as *const u64, num, ss, ps, erased.as_ptr(),
                                                  r.secrets.as_mut_ptr() as *mut u64, r.nerr.as_mut_ptr(), r.col_err.as_mut_ptr(),
                                                  r.err_mask.as_mut_ptr())
    })?;
    Ok(r)
}

/// EXTENSION: share repair over a prime below 2^256.  The decode of `shamir_reconstruct_wide_corrected` (of
/// `shamir_reconstruct_wide_erasures` when `erased` is not empty) and the corrected polynomials at the points of the parties
/// `targets`: global indices whose point `targets[j] + 1` is below p, columns of the call -- the share that party should hold --
/// or any other, duplicates allowed.  Returns `values [num_secrets][targets.len()]` (the row of an undecodable secret is 0) and
/// the decode's report (`pvw_shamir_evaluate_wide_corrected` / `pvw_shamir_evaluate_wide_erasures`).
pub fn shamir_evaluate_wide_corrected(params: &Arc<PvwParameters>, indices: &[u64], shares: &[Wide], degree: u32, plain_modulus: &Wide,
                                      erased: &[u64], targets: &[u64], party_major: bool) -> Result<(Vec<Wide>, CorrectedWideSecrets)> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and secret".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let words = (count + 63) / 64;
    if !erased.is_empty() && erased.len() != num * words {
        return Err(PvwError::InvalidParameters("erased must hold ceil(count / 64) words per secret".into()));
    }
    let er = if erased.is_empty() { std::ptr::null() } else { erased.as_ptr() };
    let mut values = vec![[0u64; 4]; num * targets.len()];
    let mut r = CorrectedWideSecrets { secrets: vec![[0u64; 4]; num], nerr: vec![0u32; num], col_err: vec![0u32; count],
                                       err_mask: vec![0u64; num * words], words };
    check(unsafe {
        sys::pvw_shamir_evaluate_wide_erasures(params.hip.raw(), plain_modulus.as_ptr(), degree, indices.as_ptr(), count,
                                               shares.as_ptr() as *const u64, num, ss, ps, er, targets.as_ptr(), targets.len(),
                                               values.as_mut_ptr() as *mut u64, r.secrets.as_mut_ptr() as *mut u64, r.nerr.as_mut_ptr(),
                                               r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok((values, r))
}

/// EXTENSION: packed shares over an odd prime below 2^256.  `secrets` is `[dealers][pack]`, dealer-major: the
/// `pack` secrets of a dealer sit at the points 0, -1, .., -(pack-1) of one polynomial with `degree` random coefficients, drawn as
/// `shamir_shares_wide` draws them or given as `coeffs [dealers][degree]`.  Returns `[dealers][n]` (`pvw_shamir_shares_packed_wide`).
pub fn shamir_shares_packed_wide(params: &Arc<PvwParameters>, secrets: &[Wide], pack: u32, degree: u32, plain_modulus: &Wide,
                                 seeds: Option<&[u8]>, coeffs: Option<&[Wide]>) -> Result<Vec<Wide>> {
    if pack == 0 || secrets.len() % pack as usize != 0 {
        return Err(PvwError::InvalidParameters("secrets must hold pack elements per dealer".into()));
    }
    let dealers = secrets.len() / pack as usize;
    let mut out = vec![[0u64; 4]; dealers * params.n];
    check(unsafe {
        sys::pvw_shamir_shares_packed_wide(params.hip.raw(), secrets.as_ptr() as *const u64, dealers, pack, degree, plain_modulus.as_ptr(),
                                           seeds.map_or(std::ptr::null(), |s| s.as_ptr()),
                                           coeffs.map_or(std::ptr::null(), |c| c.as_ptr() as *const u64), out.as_mut_ptr() as *mut u64)
    })?;
    Ok(out)
}

/// EXTENSION: `deal_party_shares_wide` with `pack` secrets per dealer in one polynomial
/// (`pvw_deal_shares_packed_wide`): `dealers * NL` ciphertexts carry `dealers * pack` wide secrets.  One seed per ciphertext comes
/// from `thread_rng` and is cleared afterwards.
pub fn deal_party_shares_packed_wide(secrets: &[Wide], pack: u32, degree: u32, plain_modulus: &Wide, limb_bits: u32,
                                     global_pk: &GlobalPublicKey) -> Result<Vec<PvwCiphertext>> {
    if pack == 0 || secrets.len() % pack as usize != 0 {
        return Err(PvwError::InvalidParameters("secrets must hold pack elements per dealer".into()));
    }
    let params = &global_pk.params;
    let dealers = secrets.len() / pack as usize;
    let vectors = dealers * shamir_wide_limbs(plain_modulus, limb_bits)? as usize;
    let words = poly_words(params);
    let mut seeds = vec![0u8; 32 * vectors];
    rand::thread_rng().fill_bytes(&mut seeds);
    let (mut c1, mut c2) = (vec![0u64; vectors * params.k * words], vec![0u64; vectors * params.n * words]);
    let rc = unsafe {
        sys::pvw_deal_shares_packed_wide(params.hip.raw(), secrets.as_ptr() as *const u64, dealers, pack, degree, plain_modulus.as_ptr(),
                                         limb_bits, seeds.as_ptr(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    };
    seeds.zeroize();
    check(rc)?;
    wide_ciphertexts(&c1, &c2, vectors, params)
}

/// `deal_party_shares_packed_wide` with vector v's randomness drawn from a `DeviceRandomness` (`call_seed(S, c + v)`).
pub fn deal_party_shares_packed_wide_with(secrets: &[Wide], pack: u32, degree: u32, plain_modulus: &Wide, limb_bits: u32,
                                          global_pk: &GlobalPublicKey, rnd: &DeviceRandomness) -> Result<Vec<PvwCiphertext>> {
    if pack == 0 || secrets.len() % pack as usize != 0 {
        return Err(PvwError::InvalidParameters("secrets must hold pack elements per dealer".into()));
    }
    let params = &global_pk.params;
    let dealers = secrets.len() / pack as usize;
    let vectors = dealers * shamir_wide_limbs(plain_modulus, limb_bits)? as usize;
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; vectors * params.k * words], vec![0u64; vectors * params.n * words]);
    check(unsafe {
        sys::pvw_deal_shares_packed_wide_rs(params.hip.raw(), secrets.as_ptr() as *const u64, dealers, pack, degree, plain_modulus.as_ptr(),
                                            limb_bits, rnd.raw(), c1.as_mut_ptr(), c2.as_mut_ptr(), sys::PVW_REPR_POWER)
    })?;
    wide_ciphertexts(&c1, &c2, vectors, params)
}

/// EXTENSION: `[num_rows][pack]`: every row's values at 0, -1, .., -(pack-1) from the shares
/// `[num_rows][indices.len()]` of the parties `indices` (at least degree + pack of them).  Host only
/// (`pvw_shamir_reconstruct_packed_wide`).
pub fn shamir_reconstruct_packed_wide(indices: &[u64], shares: &[Wide], plain_modulus: &Wide, pack: u32) -> Result<Vec<Wide>> {
    if indices.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and row".into()));
    }
    let rows = shares.len() / indices.len();
    let mut out = vec![[0u64; 4]; rows * pack.max(1) as usize];
    check(unsafe {
        sys::pvw_shamir_reconstruct_packed_wide(plain_modulus.as_ptr(), pack, indices.as_ptr(), shares.as_ptr() as *const u64, indices.len(),
                                                rows, out.as_mut_ptr() as *mut u64)
    })?;
    Ok(out)
}

/// EXTENSION: the secrets `[num_rows][pack]` of a packed wide sharing although up to
/// `(indices.len() - degree - pack) / 2` shares of each row are wrong.  The wide evaluate calls take targets as party indices, so
/// the points -j cannot be named for a wide p: ONE `shamir_evaluate_wide_corrected` call at polynomial degree `degree + pack - 1`
/// evaluates the corrected polynomials at the first `degree + pack` of `indices`, and `shamir_reconstruct_packed_wide` reads the
/// secrets off those corrected shares.  A row reported `PVW_SHAMIR_UNDECODABLE` gives `pack` zero elements; the report passes
/// through unchanged.  `pack = 1` is `shamir_reconstruct_wide_corrected`.
pub fn shamir_reconstruct_packed_wide_corrected(params: &Arc<PvwParameters>, plain_modulus: &Wide, pack: u32, degree: u32, indices: &[u64],
                                                shares: &[Wide], erased: &[u64], party_major: bool) -> Result<(Vec<Wide>, CorrectedWideSecrets)> {
    if pack == 0 {
        return Err(PvwError::InvalidParameters("pack must be at least 1".into()));
    }
    let need = degree as usize + pack as usize;
    if indices.len() < need {
        return Err(PvwError::InvalidParameters("degree + pack shares are needed".into()));
    }
    let basis = &indices[..need];
    let (values, report) = shamir_evaluate_wide_corrected(params, indices, shares, degree + pack - 1, plain_modulus, erased, basis, party_major)?;
    let mut secrets = shamir_reconstruct_packed_wide(basis, &values, plain_modulus, pack)?;
    for (r, &e) in report.nerr.iter().enumerate() {
        if e == sys::PVW_SHAMIR_UNDECODABLE {
            secrets[r * pack as usize..(r + 1) * pack as usize].iter_mut().for_each(|s| *s = [0u64; 4]);
        }
    }
    Ok((secrets, report))
}

/// EXTENSION: `shamir_evaluate_wide_corrected` with the point of column `j` of the values given as the field
/// element `points[j]`, which must be below p: 0 (the value is then the secret), points above 2^64 and points on columns are
/// legal (`pvw_shamir_evaluate_wide_erasures_at`; an empty `erased` is the corrected call).
pub fn shamir_evaluate_wide_corrected_at(params: &Arc<PvwParameters>, indices: &[u64], shares: &[Wide], degree: u32, plain_modulus: &Wide,
                                         erased: &[u64], points: &[Wide], party_major: bool) -> Result<(Vec<Wide>, CorrectedWideSecrets)> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and secret".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let words = (count + 63) / 64;
    if !erased.is_empty() && erased.len() != num * words {
        return Err(PvwError::InvalidParameters("erased must hold ceil(count / 64) words per secret".into()));
    }
    let er = if erased.is_empty() { std::ptr::null() } else { erased.as_ptr() };
    let mut values = vec![[0u64; 4]; num * points.len()];
    let mut r = CorrectedWideSecrets { secrets: vec![[0u64; 4]; num], nerr: vec![0u32; num], col_err: vec![0u32; count],
                                       err_mask: vec![0u64; num * words], words };
    check(unsafe {
        sys::pvw_shamir_evaluate_wide_erasures_at(params.hip.raw(), plain_modulus.as_ptr(), degree, indices.as_ptr(), count,
                                                  shares.as_ptr() as *const u64, num, ss, ps, er, points.as_ptr() as *const u64,
                                                  points.len(), values.as_mut_ptr() as *mut u64, r.secrets.as_mut_ptr() as *mut u64,
                                                  r.nerr.as_mut_ptr(), r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok((values, r))
}

/// EXTENSION: the secrets `[num_rows][pack]` of a packed wide sharing in ONE device call, with shares wrong or
/// erased: the rows are decoded at polynomial degree `degree + pack - 1` and read at the points `-m`
/// (`pvw_shamir_packed_wide_secrets`).  Every index must be below `p - pack`.  The report's `secrets` stays empty.
pub fn shamir_packed_wide_secrets(params: &Arc<PvwParameters>, plain_modulus: &Wide, pack: u32, degree: u32, indices: &[u64],
                                  shares: &[Wide], erased: &[u64], party_major: bool) -> Result<(Vec<Wide>, CorrectedWideSecrets)> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one element per index and row".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let words = (count + 63) / 64;
    if !erased.is_empty() && erased.len() != num * words {
        return Err(PvwError::InvalidParameters("erased must hold ceil(count / 64) words per row".into()));
    }
    let er = if erased.is_empty() { std::ptr::null() } else { erased.as_ptr() };
    let mut secrets = vec![[0u64; 4]; num * pack.max(1) as usize];
    let mut r = CorrectedWideSecrets { secrets: Vec::new(), nerr: vec![0u32; num], col_err: vec![0u32; count],
                                       err_mask: vec![0u64; num * words], words };
    check(unsafe {
        sys::pvw_shamir_packed_wide_secrets(params.hip.raw(), plain_modulus.as_ptr(), pack, degree, indices.as_ptr(), count,
                                            shares.as_ptr() as *const u64, num, ss, ps, er, secrets.as_mut_ptr() as *mut u64,
                                            r.nerr.as_mut_ptr(), r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok((secrets, r))
}

/// EXTENSION: the erasure mask of wide shares from a per-limb decrypt report, on the host
/// (`pvw_shamir_wide_erasure_mask_host`).  `status` and `noise` are `[num_secrets][count * num_limbs]`, or with `party_major`
/// `[count][num_secrets * num_limbs]` (the `[party][dealer * NL + w]` report of the decrypt-all calls, every dealer a secret);
/// either may be empty, not both.  Share `(s, c)` is erased iff one of its limbs has `status & status_bits != 0` or
/// `noise > noise_bound`.
pub fn shamir_wide_erasure_mask(status: &[u32], noise: &[u64], count: usize, num_limbs: u32, status_bits: u32, noise_bound: u64,
                                party_major: bool) -> Result<Vec<u64>> {
    let cells = if status.is_empty() { noise.len() } else { status.len() };
    let nl = num_limbs as usize;
    if count == 0 || nl == 0 || cells == 0 || cells % (count * nl) != 0 || (!status.is_empty() && !noise.is_empty() && status.len() != noise.len()) {
        return Err(PvwError::InvalidParameters("status and noise must hold num_limbs values per share".into()));
    }
    let num = cells / (count * nl);
    let (ss, ps) = if party_major { (nl, num * nl) } else { (count * nl, nl) };
    let mut mask = vec![0u64; num * ((count + 63) / 64)];
    check(unsafe {
        sys::pvw_shamir_wide_erasure_mask_host(if status.is_empty() { std::ptr::null_mut() } else { status.as_ptr() as *mut u32 },   // only read
                                               if noise.is_empty() { std::ptr::null() } else { noise.as_ptr() }, status_bits, noise_bound,
                                               count, num, ss, ps, num_limbs, 1, mask.as_mut_ptr())
    })?;
    Ok(mask)
}

/// EXTENSION: `shamir_wide_from_limbs` where the limbs lie (`pvw_shamir_wide_from_limbs_device`): device
/// pointers, `count` elements of `[count][4]` words written at `d_out`, asynchronous on `stream` (null: the context's).
/// Strides `(count, 1)` read limb planes, `(1, num_limbs)` the `[party][dealer * NL + w]` result of a decrypt-all in place.
///
/// # Safety
/// `d_limbs` and `d_out` must be device buffers that hold what the strides reach and `count * 4` words.
pub unsafe fn shamir_wide_from_limbs_device(params: &Arc<PvwParameters>, plain_modulus: &Wide, d_limbs: *const u64, count: usize,
                                            limb_stride: usize, elem_stride: usize, limb_bits: u32, num_limbs: u32, d_out: *mut u64,
                                            stream: *mut std::ffi::c_void) -> Result<()> {
    check(sys::pvw_shamir_wide_from_limbs_device(params.hip.raw(), plain_modulus.as_ptr(), d_limbs, count, limb_stride, elem_stride,
                                                 limb_bits, num_limbs, d_out, stream))
}

/// The share matrix of the checked, corrected and evaluate calls: (columns, secrets, secret stride, point stride), in words.
fn share_matrix(indices: &[u64], shares: &[u64], party_major: bool) -> Result<(usize, usize, usize, usize)> {
    if indices.is_empty() || shares.is_empty() || shares.len() % indices.len() != 0 {
        return Err(PvwError::InvalidParameters("shares must hold one value per index and secret".into()));
    }
    let (count, num) = (indices.len(), shares.len() / indices.len());
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    Ok((count, num, ss, ps))
}

/// EXTENSION: what `shamir_reconstruct_checked` reports.
pub struct CheckedSecrets {
    /// the value at 0 of the polynomial through each secret's basis shares
    pub secrets: Vec<u64>,
    /// per secret: columns beyond the basis whose share is off that polynomial
    pub bad: Vec<u32>,
    /// per column: secrets that deviate there (0 for the basis columns)
    pub col_bad: Vec<u32>,
}

/// EXTENSION: the secrets and a report on the shares, on the device (`pvw_shamir_reconstruct_checked`).  The
/// first `degree + 1` of `indices` are the basis.  `shares` is `[num_secrets][indices.len()]` row-major, or with
/// `party_major` `[indices.len()][num_secrets]` (what `decrypt_all_party_shares` returns, every dealer a secret).
pub fn shamir_reconstruct_checked(params: &Arc<PvwParameters>, indices: &[u64], shares: &[u64], degree: u32, plain_modulus: u64,
                                  party_major: bool) -> Result<CheckedSecrets> {
    let (count, num, ss, ps) = share_matrix(indices, shares, party_major)?;
    let mut r = CheckedSecrets { secrets: vec![0u64; num], bad: vec![0u32; num], col_bad: vec![0u32; count] };
    check(unsafe {
        sys::pvw_shamir_reconstruct_checked(params.hip.raw(), plain_modulus, degree, indices.as_ptr(), count, shares.as_ptr(), num, ss, ps,
                                            r.secrets.as_mut_ptr(), r.bad.as_mut_ptr(), r.col_bad.as_mut_ptr())
    })?;
    Ok(r)
}

/// EXTENSION: what `shamir_reconstruct_corrected` reports.
pub struct CorrectedSecrets {
    /// the value at 0 of the one polynomial within E columns of each row; 0 for an undecodable row
    pub secrets: Vec<u64>,
    /// per secret: columns off that polynomial, or `sys::PVW_SHAMIR_UNDECODABLE`
    pub nerr: Vec<u32>,
    /// per column: decodable secrets that are off there
    pub col_err: Vec<u32>,
    /// `[num_secrets][words]`: bit `c % 64` of word `c / 64` names the columns counted in `nerr`
    pub err_mask: Vec<u64>,
    /// `ceil(indices.len() / 64)`
    pub words: usize,
}

impl CorrectedSecrets {
    fn zeroed(count: usize, num: usize) -> Self {
        let words = (count + 63) / 64;
        CorrectedSecrets { secrets: vec![0u64; num], nerr: vec![0u32; num], col_err: vec![0u32; count], err_mask: vec![0u64; num * words], words }
    }
}

/// EXTENSION: the secrets although up to `(indices.len() - degree - 1) / 2` shares of each are wrong, in
/// whichever columns, on the device (`pvw_shamir_reconstruct_corrected`).  `shares` as `shamir_reconstruct_checked`.
pub fn shamir_reconstruct_corrected(params: &Arc<PvwParameters>, indices: &[u64], shares: &[u64], degree: u32, plain_modulus: u64,
                                    party_major: bool) -> Result<CorrectedSecrets> {
    let (count, num, ss, ps) = share_matrix(indices, shares, party_major)?;
    let mut r = CorrectedSecrets::zeroed(count, num);
    check(unsafe {
        sys::pvw_shamir_reconstruct_corrected(params.hip.raw(), plain_modulus, degree, indices.as_ptr(), count, shares.as_ptr(), num, ss, ps,
                                              r.secrets.as_mut_ptr(), r.nerr.as_mut_ptr(), r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok(r)
}

/// EXTENSION: share repair on the device (`pvw_shamir_evaluate_corrected`).  The decode of
/// `shamir_reconstruct_corrected` and, as `[num_secrets][targets.len()]`, every row's corrected polynomial at the points of the
/// parties `targets` (global indices, among `indices` or not; duplicates allowed).  The row of an undecodable secret is 0.
pub fn shamir_evaluate_corrected(params: &Arc<PvwParameters>, indices: &[u64], shares: &[u64], degree: u32, plain_modulus: u64,
                                 targets: &[u64], party_major: bool) -> Result<(Vec<u64>, CorrectedSecrets)> {
    let (count, num, ss, ps) = share_matrix(indices, shares, party_major)?;
    let mut values = vec![0u64; num * targets.len()];
    let mut r = CorrectedSecrets::zeroed(count, num);
    check(unsafe {
        sys::pvw_shamir_evaluate_corrected(params.hip.raw(), plain_modulus, degree, indices.as_ptr(), count, shares.as_ptr(), num, ss, ps,
                                           targets.as_ptr(), targets.len(), values.as_mut_ptr(), r.secrets.as_mut_ptr(), r.nerr.as_mut_ptr(),
                                           r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok((values, r))
}

/// The mask rows of a call with erasures: `[num_secrets][ceil(count / 64)]` words in the layout of `CorrectedSecrets::err_mask`.
fn erased_rows(erased: &[u64], count: usize, num: usize) -> Result<*const u64> {
    if erased.len() != num * ((count + 63) / 64) {
        return Err(PvwError::InvalidParameters("erased must hold ceil(count / 64) words per secret".into()));
    }
    Ok(erased.as_ptr())
}

/// EXTENSION: `shamir_reconstruct_corrected` with the shares KNOWN to be bad flagged in `erased` (bit `c % 64` of
/// word `c / 64` of row `s`; an earlier call's `err_mask`, or `shamir_erasure_mask`).  Each costs one redundant column instead of
/// two: a row decodes while `2 * errors + erasures <= indices.len() - degree - 1`.  The word at an erased position influences nothing
/// and an erased column is never reported as an error (`pvw_shamir_reconstruct_erasures`).
pub fn shamir_reconstruct_erasures(params: &Arc<PvwParameters>, indices: &[u64], shares: &[u64], degree: u32, plain_modulus: u64,
                                   erased: &[u64], party_major: bool) -> Result<CorrectedSecrets> {
    let (count, num, ss, ps) = share_matrix(indices, shares, party_major)?;
    let er = erased_rows(erased, count, num)?;
    let mut r = CorrectedSecrets::zeroed(count, num);
    check(unsafe {
        sys::pvw_shamir_reconstruct_erasures(params.hip.raw(), plain_modulus, degree, indices.as_ptr(), count, shares.as_ptr(), num, ss, ps, er,
                                             r.secrets.as_mut_ptr(), r.nerr.as_mut_ptr(), r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok(r)
}

/// EXTENSION: `shamir_evaluate_corrected` with erasures (`pvw_shamir_evaluate_erasures`).  At an erased or wrong
/// column the value is the share that party should hold: the repair of a party that lost its state.
pub fn shamir_evaluate_erasures(params: &Arc<PvwParameters>, indices: &[u64], shares: &[u64], degree: u32, plain_modulus: u64,
                                erased: &[u64], targets: &[u64], party_major: bool) -> Result<(Vec<u64>, CorrectedSecrets)> {
    let (count, num, ss, ps) = share_matrix(indices, shares, party_major)?;
    let er = erased_rows(erased, count, num)?;
    let mut values = vec![0u64; num * targets.len()];
    let mut r = CorrectedSecrets::zeroed(count, num);
    check(unsafe {
        sys::pvw_shamir_evaluate_erasures(params.hip.raw(), plain_modulus, degree, indices.as_ptr(), count, shares.as_ptr(), num, ss, ps, er,
                                          targets.as_ptr(), targets.len(), values.as_mut_ptr(), r.secrets.as_mut_ptr(), r.nerr.as_mut_ptr(),
                                          r.col_err.as_mut_ptr(), r.err_mask.as_mut_ptr())
    })?;
    Ok((values, r))
}

/// EXTENSION: the erasure mask of a decrypt report, on the host (`pvw_shamir_erasure_mask_host`).  `status` and
/// `noise` are `[num_secrets][count]`, or with `party_major` `[count][num_secrets]` (the `[party][dealer]` report of the
/// decrypt-all calls, every dealer a secret); either may be empty, not both.  Share `(s, c)` is erased iff
/// `status & status_bits != 0` or `noise > noise_bound`.
pub fn shamir_erasure_mask(status: &[u32], noise: &[u64], count: usize, status_bits: u32, noise_bound: u64, party_major: bool) -> Result<Vec<u64>> {
    let cells = if status.is_empty() { noise.len() } else { status.len() };
    if count == 0 || cells == 0 || cells % count != 0 || (!status.is_empty() && !noise.is_empty() && status.len() != noise.len()) {
        return Err(PvwError::InvalidParameters("status and noise must hold one value per share".into()));
    }
    let num = cells / count;
    let (ss, ps) = if party_major { (1, num) } else { (count, 1) };
    let mut mask = vec![0u64; num * ((count + 63) / 64)];
    check(unsafe {
        sys::pvw_shamir_erasure_mask_host(if status.is_empty() { std::ptr::null_mut() } else { status.as_ptr() as *mut u32 },   // only read
                                          if noise.is_empty() { std::ptr::null() } else { noise.as_ptr() }, status_bits, noise_bound, count, num, ss,
                                          ps, mask.as_mut_ptr())
    })?;
    Ok(mask)
}

/// EXTENSION: the sum of the valid dealers' ciphertexts (`pvw_ct_sum`) -- a ciphertext of the sum of their
/// shares under the same keys, folded without any key.  What examples/pvw_valid_dec.rs:150-209 reaches by decrypting every
/// dealer's share and adding the results; the noise of the sum is the sum of the dealers' noises (`pvw_ctx_sum_capacity`).
pub fn aggregate_ciphertexts(ciphertexts: &[PvwCiphertext], valid: Option<&[bool]>) -> Result<PvwCiphertext> {
    let (c1s, c2s, v) = sum_inputs(ciphertexts, valid)?;
    let params = &ciphertexts[0].params;
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; params.k * words], vec![0u64; params.n * words]);
    check(unsafe {
        sys::pvw_ct_sum(params.hip.raw(), c1s.as_ptr(), c2s.as_ptr(), ciphertexts.len(), valid_ptr(&v), 0, params.n as u32, c1.as_mut_ptr(),
                        c2.as_mut_ptr(), std::ptr::null_mut())
    })?;
    ciphertext_from_flat(&c1, &c2, params)
}

/// EXTENSION: party `party_index`'s aggregate share from ONE decrypt of the summed ciphertext (`pvw_decrypt_sum_checked`):
/// (value, noise, lossy, dealers summed).  `noise` is the exact max residual of the aggregate.
pub fn decrypt_party_sum(ciphertexts: &[PvwCiphertext], secret_key: &SecretKey, party_index: usize, valid: Option<&[bool]>) -> Result<(u64, u64, bool, u32)> {
    let (r, count) = decrypt_party_sum_plain(ciphertexts, secret_key, party_index, valid, &PlainOptions::default())?;
    Ok((r.values[0], r.noise[0], r.status[0] & sys::PVW_DEC_LOSSY != 0, count))
}

/// EXTENSION: `decrypt_party_sum` with the plain options (`pvw_decrypt_sum_plain`): the sum of the party's shares
/// mod `plain.modulus` and / or as wide words -- exact where the u64 word of a field-sized sum is 0.  (report of one share,
/// dealers summed)
pub fn decrypt_party_sum_plain(ciphertexts: &[PvwCiphertext], secret_key: &SecretKey, party_index: usize, valid: Option<&[bool]>, plain: &PlainOptions) -> Result<(PlainDecryption, u32)> {
    let (c1s, c2s, v) = sum_inputs(ciphertexts, valid)?;
    let params = &ciphertexts[0].params;
    if party_index >= params.n {
        return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party_index, params.n - 1)));
    }
    let words = poly_words(params);
    let c2col: Vec<u64> = c2s.chunks_exact(params.n * words).flat_map(|ct| ct[party_index * words..(party_index + 1) * words].to_vec()).collect();
    let mut sk = flat_secret(secret_key);
    let (mut out, mut noise, mut status, mut count) = (0u64, 0u64, 0u32, 0u32);
    let mut wide = vec![0u64; plain.wide_words as usize];
    let rc = unsafe {
        sys::pvw_decrypt_sum_plain(params.hip.raw(), sk.as_ptr(), c1s.as_ptr(), c2col.as_ptr(), ciphertexts.len(), valid_ptr(&v),
                                   sys::PVW_REPR_POWER, &mut out, &mut noise, &mut status, &mut count, plain.modulus, plain.wide_words,
                                   wide_ptr(&mut wide))
    };
    sk.zeroize();
    check(rc)?;
    Ok((PlainDecryption { values: vec![out], noise: vec![noise], status: vec![status], wide }, count))
}

/// EXTENSION: every party's aggregate share in one call (`pvw_decrypt_all_sum_checked`): (values, noise, lossy) per party.
/// `parties` must carry consecutive indices.
pub fn decrypt_all_party_sums(ciphertexts: &[PvwCiphertext], parties: &[crate::keys::public_key::Party], valid: Option<&[bool]>) -> Result<(Vec<u64>, Vec<u64>, Vec<bool>)> {
    let r = decrypt_all_party_sums_plain(ciphertexts, parties, valid, &PlainOptions::default())?;
    Ok((r.values, r.noise, r.status.iter().map(|s| s & sys::PVW_DEC_LOSSY != 0).collect()))
}

/// EXTENSION: `decrypt_all_party_sums` with the plain options (`pvw_decrypt_all_sum_plain`); wide is
/// [parties][wide_words].
pub fn decrypt_all_party_sums_plain(ciphertexts: &[PvwCiphertext], parties: &[crate::keys::public_key::Party], valid: Option<&[bool]>, plain: &PlainOptions) -> Result<PlainDecryption> {
    let (c1s, c2s, v) = sum_inputs(ciphertexts, valid)?;
    let params = &ciphertexts[0].params;
    if parties.is_empty() {
        return Ok(PlainDecryption::default());
    }
    let lo = parties[0].index;
    for (i, party) in parties.iter().enumerate() {
        if party.index >= params.n {
            return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party.index, params.n - 1)));
        }
        if party.index != lo + i {
            return Err(PvwError::InvalidParameters(format!("Party indices must be consecutive: {} follows {}", party.index, lo + i - 1)));
        }
    }
    let mut sk: Vec<i64> = parties.iter().flat_map(|p| flat_secret(&p.secret_key)).collect();
    let np = parties.len();
    let (mut out, mut noise, mut status) = (vec![0u64; np], vec![0u64; np], vec![0u32; np]);
    let mut wide = vec![0u64; np * plain.wide_words as usize];
    let rc = unsafe {
        sys::pvw_decrypt_all_sum_plain(params.hip.raw(), lo as u32, (lo + np) as u32, sk.as_ptr(), c1s.as_ptr(), c2s.as_ptr(), ciphertexts.len(),
                                       valid_ptr(&v), sys::PVW_REPR_POWER, out.as_mut_ptr(), noise.as_mut_ptr(), status.as_mut_ptr(),
                                       std::ptr::null_mut(), plain.modulus, plain.wide_words, wide_ptr(&mut wide))
    };
    sk.zeroize();
    check(rc)?;
    Ok(PlainDecryption { values: out, noise, status, wide })
}

/// The weights of a combination next to its ciphertexts: one per dealer.
fn combination_weights(ciphertexts: &[PvwCiphertext], weights: &[i64]) -> Result<()> {
    if weights.len() != ciphertexts.len() {
        return Err(PvwError::DimensionMismatch { expected: ciphertexts.len(), actual: weights.len() });
    }
    Ok(())
}

/// EXTENSION: the weighted sum of the dealers' ciphertexts (`pvw_ct_lincomb`) -- a ciphertext of
/// sum_d w_d m_d under the same keys, with noise sum_d |w_d| noise_d (`pvw_ctx_lincomb_fits`).  A dealer takes part when it
/// is valid and its weight is not 0.
pub fn combine(ciphertexts: &[PvwCiphertext], weights: &[i64], valid: Option<&[bool]>) -> Result<PvwCiphertext> {
    let (c1s, c2s, v) = sum_inputs(ciphertexts, valid)?;
    combination_weights(ciphertexts, weights)?;
    let params = &ciphertexts[0].params;
    let words = poly_words(params);
    let (mut c1, mut c2) = (vec![0u64; params.k * words], vec![0u64; params.n * words]);
    check(unsafe {
        sys::pvw_ct_lincomb(params.hip.raw(), c1s.as_ptr(), c2s.as_ptr(), ciphertexts.len(), valid_ptr(&v), weights.as_ptr(), 0,
                            params.n as u32, c1.as_mut_ptr(), c2.as_mut_ptr(), std::ptr::null_mut())
    })?;
    ciphertext_from_flat(&c1, &c2, params)
}

/// EXTENSION: row j = the Lagrange weights AT the point (targets[j] + 1) mod p of the points indices[i] + 1,
/// centred in (-p/2, p/2] (`pvw_shamir_lagrange_weights_at`; host only).  Target p - 1 - m is the point -m of a packed sharing.
pub fn shamir_lagrange_weights_at(indices: &[u64], targets: &[u64], plain_modulus: u64) -> Result<Vec<Vec<i64>>> {
    let mut flat = vec![0i64; indices.len() * targets.len()];
    check(unsafe {
        sys::pvw_shamir_lagrange_weights_at(plain_modulus, indices.as_ptr(), indices.len(), targets.as_ptr(), targets.len(), flat.as_mut_ptr())
    })?;
    Ok(flat.chunks(indices.len().max(1)).map(|row| row.to_vec()).collect())
}

/// EXTENSION: one combination per row of `weight_rows` over the same ciphertexts (`pvw_ct_lincomb_many`): element
/// r is `combine(ciphertexts, &weight_rows[r], valid)` bit for bit, zeros for a row nobody takes part in; every ciphertext is
/// uploaded once and read once per tile of rows.
pub fn combine_many(ciphertexts: &[PvwCiphertext], weight_rows: &[Vec<i64>], valid: Option<&[bool]>) -> Result<Vec<PvwCiphertext>> {
    let (c1s, c2s, v) = sum_inputs(ciphertexts, valid)?;
    let mut weights = Vec::with_capacity(weight_rows.len() * ciphertexts.len());
    for row in weight_rows {
        combination_weights(ciphertexts, row)?;
        weights.extend_from_slice(row);
    }
    let params = &ciphertexts[0].params;
    let (words, rows) = (poly_words(params), weight_rows.len());
    let (mut c1, mut c2) = (vec![0u64; rows * params.k * words], vec![0u64; rows * params.n * words]);
    check(unsafe {
        sys::pvw_ct_lincomb_many(params.hip.raw(), c1s.as_ptr(), c2s.as_ptr(), ciphertexts.len(), valid_ptr(&v), weights.as_ptr(), rows, 0,
                                 params.n as u32, c1.as_mut_ptr(), c2.as_mut_ptr(), std::ptr::null_mut())
    })?;
    c1.chunks_exact(params.k * words).zip(c2.chunks_exact(params.n * words)).map(|(a, b)| ciphertext_from_flat(a, b, params)).collect()
}

/// EXTENSION: party `party_index`'s share of the combination from ONE decrypt (`pvw_decrypt_lincomb_plain`), with the plain
/// options of DESIGN 8.8: with the Lagrange weights of the valid old holders and `plain.modulus` = p this is the party's new
/// share after a committee handover.  (report of one share, dealers that took part)
pub fn decrypt_combination(ciphertexts: &[PvwCiphertext], weights: &[i64], secret_key: &SecretKey, party_index: usize, valid: Option<&[bool]>, plain: &PlainOptions) -> Result<(PlainDecryption, u32)> {
    let (c1s, c2s, v) = sum_inputs(ciphertexts, valid)?;
    combination_weights(ciphertexts, weights)?;
    let params = &ciphertexts[0].params;
    if party_index >= params.n {
        return Err(PvwError::InvalidParameters(format!("Party index {} exceeds maximum {}", party_index, params.n - 1)));
    }
    let words = poly_words(params);
    let c2col: Vec<u64> = c2s.chunks_exact(params.n * words).flat_map(|ct| ct[party_index * words..(party_index + 1) * words].to_vec()).collect();
    let mut sk = flat_secret(secret_key);
    let (mut out, mut noise, mut status, mut count) = (0u64, 0u64, 0u32, 0u32);
    let mut wide = vec![0u64; plain.wide_words as usize];
    let rc = unsafe {
        sys::pvw_decrypt_lincomb_plain(params.hip.raw(), sk.as_ptr(), c1s.as_ptr(), c2col.as_ptr(), ciphertexts.len(), valid_ptr(&v),
                                       weights.as_ptr(), sys::PVW_REPR_POWER, &mut out, &mut noise, &mut status, &mut count,
                                       plain.modulus, plain.wide_words, wide_ptr(&mut wide))
    };
    sk.zeroize();
    check(rc)?;
    Ok((PlainDecryption { values: vec![out], noise: vec![noise], status: vec![status], wide }, count))
}

/// EXTENSION: (NL, V) of a wide handover: the limbs of a share and the signed digits of a weight,
/// V = ceil((bitlen(p) + 1) / digit_bits) (`pvw_shamir_wide_handover_shape`; host only).
pub fn shamir_wide_handover_shape(plain_modulus: &Wide, limb_bits: u32, digit_bits: u32) -> Result<(u32, u32)> {
    let (mut nl, mut nd) = (0u32, 0u32);
    check(unsafe { sys::pvw_shamir_wide_handover_shape(plain_modulus.as_ptr(), limb_bits, digit_bits, &mut nl, &mut nd) })?;
    Ok((nl, nd))
}

/// EXTENSION: the signed digits `[values.len()][V]` of the centred residues of `values` mod p, every digit in
/// [-2^(digit_bits-1), 2^(digit_bits-1)) (`pvw_shamir_wide_signed_digits_host`).
pub fn shamir_wide_signed_digits(values: &[Wide], plain_modulus: &Wide, digit_bits: u32) -> Result<Vec<i64>> {
    let (_, nd) = shamir_wide_handover_shape(plain_modulus, 62, digit_bits)?;
    let mut out = vec![0i64; values.len() * nd as usize];
    check(unsafe {
        sys::pvw_shamir_wide_signed_digits_host(plain_modulus.as_ptr(), values.as_ptr() as *const u64, values.len(), digit_bits, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// EXTENSION: the points 0, -1, .., -(pack-1) of a packed wide sharing as field elements (-m is p - m).
pub fn shamir_packed_wide_handover_points(plain_modulus: &Wide, pack: u32) -> Vec<Wide> {
    (0..pack as u64).map(|m| {
        let mut out = [0u64; 4];
        if m != 0 {
            let mut br = m;
            for i in 0..4 {
                let v = plain_modulus[i];
                out[i] = v.wrapping_sub(br);
                br = (v < br) as u64;
            }
        }
        out
    }).collect()
}

fn handover_valid(valid: Option<&[bool]>, holders: usize) -> Result<Vec<u8>> {
    match valid {
        Some(v) if v.len() != holders => Err(PvwError::InvalidParameters("valid must hold one flag per holder".into())),
        Some(v) => Ok(v.iter().map(|&b| b as u8).collect()),
        None => Ok(Vec::new()),
    }
}

/// EXTENSION: the int64 weight rows `[T V][D NL]` of a wide handover, row m V + v, column d NL + w = signed digit v
/// of lambda_{d,m} 2^(limb_bits w) mod p; `points` empty = the single point 0 (`pvw_shamir_wide_handover_weights_host`).
pub fn shamir_wide_handover_weights(indices: &[u64], plain_modulus: &Wide, valid: Option<&[bool]>, points: &[Wide], limb_bits: u32,
                                    digit_bits: u32) -> Result<Vec<i64>> {
    let v = handover_valid(valid, indices.len())?;
    let (nl, nd) = shamir_wide_handover_shape(plain_modulus, limb_bits, digit_bits)?;
    let t = points.len().max(1);
    let mut out = vec![0i64; t * nd as usize * indices.len() * nl as usize];
    let pts = if points.is_empty() { std::ptr::null() } else { points.as_ptr() as *const u64 };
    check(unsafe {
        sys::pvw_shamir_wide_handover_weights_host(plain_modulus.as_ptr(), indices.as_ptr(), valid_ptr(&v), indices.len(), pts, t, limb_bits,
                                                   digit_bits, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// EXTENSION: (values, status) from digit plaintexts `wide [count][num_digits][wide_words]` and
/// `status [count][num_digits]`: values[i] = sum_v +-wide[i][v] 2^(digit_bits v) mod p, status[i] the OR of the digit words
/// without `PVW_DEC_NEGATIVE` (`pvw_shamir_wide_from_digits_host`).
pub fn shamir_wide_from_digits(wide: &[u64], status: &[u32], num_digits: u32, wide_words: u32, plain_modulus: &Wide,
                               digit_bits: u32) -> Result<(Vec<Wide>, Vec<u32>)> {
    if num_digits == 0 || wide_words == 0 || status.len() % num_digits as usize != 0 || wide.len() != status.len() * wide_words as usize {
        return Err(PvwError::InvalidParameters("wide must hold wide_words words per status word, num_digits of them per element".into()));
    }
    let count = status.len() / num_digits as usize;
    let (mut out, mut st_out) = (vec![[0u64; 4]; count], vec![0u32; count]);
    let mut st = status.to_vec();
    check(unsafe {
        sys::pvw_shamir_wide_from_digits_host(plain_modulus.as_ptr(), digit_bits, num_digits, wide.as_ptr(), st.as_mut_ptr(), wide_words, count,
                                              out.as_mut_ptr() as *mut u64, st_out.as_mut_ptr())
    })?;
    Ok((out, st_out))
}

/// EXTENSION: whether every weight row of a wide handover stays inside the radius the decode is proven exact in,
/// and its digit plaintexts fit the words of Q (`pvw_ctx_wide_handover_fits`; advisory, sufficient only).
pub fn wide_handover_fits(params: &Arc<PvwParameters>, plain_modulus: &Wide, num_valid: usize, limb_bits: u32, digit_bits: u32) -> Result<bool> {
    let mut fits = 0u32;
    check(unsafe { sys::pvw_ctx_wide_handover_fits(params.hip.raw(), plain_modulus.as_ptr(), num_valid, limb_bits, digit_bits, &mut fits) })?;
    Ok(fits != 0)
}

/// EXTENSION: every new party's new share in one call (`pvw_decrypt_all_handover_wide`).  `ciphertexts` are the old
/// holders' limb ciphertexts, vector d NL + w limb w of holder d; `secret_keys` those of the consecutive parties from `party_lo`.
/// (values `[parties][T]`, status `[parties][T]`, valid holders)
pub fn decrypt_all_party_handover_wide(ciphertexts: &[PvwCiphertext], secret_keys: &[SecretKey], party_lo: usize, indices: &[u64],
                                       plain_modulus: &Wide, valid: Option<&[bool]>, points: &[Wide], limb_bits: u32,
                                       digit_bits: u32) -> Result<(Vec<Wide>, Vec<u32>, u32)> {
    let (c1s, c2s, _) = sum_inputs(ciphertexts, None)?;
    let v = handover_valid(valid, indices.len())?;
    let nl = shamir_wide_limbs(plain_modulus, limb_bits)? as usize;
    if indices.is_empty() || ciphertexts.len() != indices.len() * nl {
        return Err(PvwError::InvalidParameters("num_limbs ciphertexts per holder".into()));
    }
    let params = &ciphertexts[0].params;
    let (np, t) = (secret_keys.len(), points.len().max(1));
    let mut sk: Vec<i64> = secret_keys.iter().flat_map(flat_secret).collect();
    let (mut out, mut status, mut count) = (vec![[0u64; 4]; np * t], vec![0u32; np * t], 0u32);
    let pts = if points.is_empty() { std::ptr::null() } else { points.as_ptr() as *const u64 };
    let rc = unsafe {
        sys::pvw_decrypt_all_handover_wide(params.hip.raw(), party_lo as u32, (party_lo + np) as u32, sk.as_ptr(), c1s.as_ptr(), c2s.as_ptr(),
                                           indices.len(), plain_modulus.as_ptr(), limb_bits, digit_bits, indices.as_ptr(), valid_ptr(&v), pts, t,
                                           sys::PVW_REPR_POWER, out.as_mut_ptr() as *mut u64, status.as_mut_ptr(), &mut count)
    };
    sk.zeroize();
    check(rc)?;
    Ok((out, status, count))
}

/// EXTENSION: the int64 weight rows `[T][D]` of a one-word handover and the number of valid holders: row j = the
/// Lagrange weights AT the point (targets[j] + 1) mod p over the holders with `valid[d]`, centred; a masked holder's column is 0;
/// `targets` empty = the single point 0 (`pvw_shamir_handover_weights_host`; the device form reads its mask from device memory
/// and is reached through the C ABI).
pub fn shamir_handover_weights(indices: &[u64], plain_modulus: u64, valid: Option<&[bool]>, targets: &[u64]) -> Result<(Vec<i64>, u32)> {
    let v = handover_valid(valid, indices.len())?;
    let t = targets.len().max(1);
    let (mut out, mut count) = (vec![0i64; t * indices.len()], 0u32);
    let tg = if targets.is_empty() { std::ptr::null() } else { targets.as_ptr() };
    check(unsafe {
        sys::pvw_shamir_handover_weights_host(plain_modulus, indices.as_ptr(), valid_ptr(&v), indices.len(), tg, t, out.as_mut_ptr(), &mut count)
    })?;
    Ok((out, count))
}

/// EXTENSION: the holder mask of a `[rows][count]` report and the number of ones: valid[c] = 1 iff no row has
/// `status & status_bits != 0` or `noise > noise_bound` in column c; either slice may be empty, not both
/// (`pvw_shamir_valid_mask_host`).
pub fn shamir_valid_mask(status: &[u32], noise: &[u64], count: usize, status_bits: u32, noise_bound: u64) -> Result<(Vec<u8>, u32)> {
    let have = if status.is_empty() { noise.len() } else { status.len() };
    if count == 0 || have % count != 0 || (!status.is_empty() && !noise.is_empty() && status.len() != noise.len()) {
        return Err(PvwError::InvalidParameters("status and noise must be [rows][count] arrays of one shape".into()));
    }
    let mut st = status.to_vec();
    let (mut out, mut num) = (vec![0u8; count], 0u32);
    let sp = if st.is_empty() { std::ptr::null_mut() } else { st.as_mut_ptr() };
    let np = if noise.is_empty() { std::ptr::null() } else { noise.as_ptr() };
    check(unsafe { sys::pvw_shamir_valid_mask_host(sp, np, status_bits, noise_bound, count, have / count, count, 1, out.as_mut_ptr(), &mut num) })?;
    Ok((out, num))
}

/// EXTENSION: every new party's new share in one call (`pvw_decrypt_all_handover`).  `ciphertexts` are the old
/// holders' re-dealt ciphertexts, holder d at party index `indices[d]`; `secret_keys` those of the consecutive parties from
/// `party_lo`.  (values `[parties][T]` mod p, noise, status, valid holders)
pub fn decrypt_all_party_handover(ciphertexts: &[PvwCiphertext], secret_keys: &[SecretKey], party_lo: usize, indices: &[u64],
                                  plain_modulus: u64, valid: Option<&[bool]>, targets: &[u64]) -> Result<(Vec<u64>, Vec<u64>, Vec<u32>, u32)> {
    let (c1s, c2s, _) = sum_inputs(ciphertexts, None)?;
    let v = handover_valid(valid, indices.len())?;
    if ciphertexts.len() != indices.len() {
        return Err(PvwError::InvalidParameters("one ciphertext per holder".into()));
    }
    let params = &ciphertexts[0].params;
    let (np, t) = (secret_keys.len(), targets.len().max(1));
    let mut sk: Vec<i64> = secret_keys.iter().flat_map(flat_secret).collect();
    let (mut out, mut noise, mut status, mut count) = (vec![0u64; np * t], vec![0u64; np * t], vec![0u32; np * t], 0u32);
    let tg = if targets.is_empty() { std::ptr::null() } else { targets.as_ptr() };
    let rc = unsafe {
        sys::pvw_decrypt_all_handover(params.hip.raw(), party_lo as u32, (party_lo + np) as u32, sk.as_ptr(), c1s.as_ptr(), c2s.as_ptr(),
                                      indices.len(), valid_ptr(&v), indices.as_ptr(), tg, t, sys::PVW_REPR_POWER, out.as_mut_ptr(),
                                      noise.as_mut_ptr(), status.as_mut_ptr(), &mut count, plain_modulus, 0, std::ptr::null_mut())
    };
    sk.zeroize();
    check(rc)?;
    Ok((out, noise, status, count))
}

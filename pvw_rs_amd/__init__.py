"""pvw_rs_amd -- MI355X-native (gfx950) PVW multi-receiver encrypt/decrypt hot path.

`csrc/` holds the hand-written HIP kernels and the C ABI (include/pvw_hip.h);
`api.py` is the host-side mirror of the reference's `pvw::{params,crs,keys,crypto}`
interface over that ABI; `host/pvw.hpp` is the same mirror in C++.
There is no CPU fallback: device entry points fail loudly without the library / a GPU.
"""
from ._ffi import (DOM_SHAMIR, DOM_CALL, DOM_CRS, DOM_E1, DOM_E2, DOM_EKEY, DOM_GAUSS, DOM_PK, DOM_R, DOM_SK, PREPARE_MFMA, PREPARE_PACKED, PREPARE_SUM,
                   REPR_NTT, REPR_POWER)
from .api import (DEC_LOSSY, DEC_NEGATIVE, DEC_WIDE_TRUNCATED, CheckedDecryption, DeviceRandomness, DeviceSecretKey, GlobalPublicKey, Party, PvwCiphertext, PvwCrs, PvwError, PvwParameters,
                  PvwParametersBuilder, SecretKey, decode_scalar_pvw, decode_scalar_pvw_host, decrypt_all_party_shares, decrypt_many,
                  decrypt_party_shares, decode_scalar_pvw_checked, decode_scalar_pvw_checked_host, decrypt_all_party_shares_checked,
                  decrypt_many_checked, decrypt_party_shares_checked, decrypt_party_value_checked,
                  decrypt_party_value, device_available, encrypt, encrypt_all_party_shares,
                  encrypt_broadcast, encrypt_many, encrypt_party_shares, aggregate_ciphertexts, decrypt_party_sum,
                  decrypt_all_party_sums, decode_scalar_pvw_plain, decode_scalar_pvw_plain_host,
                  shamir_shares, deal_party_shares, shamir_reconstruct, shamir_reconstruct_checked,
                  shamir_reconstruct_corrected, shamir_evaluate_corrected, shamir_erasure_mask, SHAMIR_UNDECODABLE, combine_ciphertexts, decrypt_party_combination,
                  decrypt_all_party_combinations, shamir_lagrange_weights, shamir_shares_packed, deal_party_shares_packed,
                  shamir_reconstruct_packed, shamir_packed_secret_indices, shamir_reconstruct_packed_corrected,
                  combine_ciphertexts_many, decrypt_all_party_combinations_many, shamir_lagrange_weights_at,
                  shamir_packed_handover_weights, sample_secret_keys_device, shamir_shares_wide, deal_party_shares_wide,
                  shamir_wide_limbs, shamir_wide_to_limbs, shamir_wide_from_limbs, shamir_reconstruct_wide,
                  shamir_wide_from_limbs_device, shamir_reconstruct_wide_checked,
                  shamir_reconstruct_wide_corrected, shamir_wide_erasure_mask, shamir_evaluate_wide_corrected,
                  shamir_shares_packed_wide, deal_party_shares_packed_wide, shamir_reconstruct_packed_wide,
                  shamir_reconstruct_packed_wide_corrected, shamir_evaluate_wide_corrected_at,
                  shamir_packed_wide_secrets, shamir_wide_handover_shape, shamir_wide_signed_digits,
                  shamir_wide_handover_weights, shamir_wide_from_digits, shamir_packed_wide_handover_points,
                  decrypt_all_party_handover_wide, shamir_handover_weights, shamir_valid_mask, decrypt_all_party_handover)

__all__ = [
    "PvwParametersBuilder", "PvwParameters", "PvwCrs", "SecretKey", "DeviceSecretKey", "DeviceRandomness", "Party", "GlobalPublicKey",
    "PvwCiphertext", "PvwError", "encrypt", "encrypt_party_shares", "encrypt_all_party_shares",
    "encrypt_broadcast", "encrypt_many", "decrypt_party_value", "decrypt_party_shares",
    "decrypt_all_party_shares", "decrypt_many", "decode_scalar_pvw",
    "CheckedDecryption", "DEC_LOSSY", "DEC_NEGATIVE", "DEC_WIDE_TRUNCATED", "decrypt_party_value_checked", "decrypt_party_shares_checked", "decrypt_many_checked",
    "decrypt_all_party_shares_checked", "decode_scalar_pvw_checked", "decode_scalar_pvw_checked_host",
    "decode_scalar_pvw_plain", "decode_scalar_pvw_plain_host",
    "aggregate_ciphertexts", "decrypt_party_sum", "decrypt_all_party_sums",
    "combine_ciphertexts", "decrypt_party_combination", "decrypt_all_party_combinations", "shamir_lagrange_weights",
    "shamir_shares_packed", "deal_party_shares_packed", "shamir_reconstruct_packed", "shamir_packed_secret_indices",
    "shamir_reconstruct_packed_corrected",
    "combine_ciphertexts_many", "decrypt_all_party_combinations_many", "shamir_lagrange_weights_at", "shamir_packed_handover_weights",
    "shamir_shares", "deal_party_shares", "shamir_reconstruct", "shamir_reconstruct_checked", "shamir_reconstruct_corrected", "shamir_evaluate_corrected", "shamir_erasure_mask", "SHAMIR_UNDECODABLE",
    "sample_secret_keys_device",
    "shamir_shares_wide", "deal_party_shares_wide", "shamir_wide_limbs", "shamir_wide_to_limbs", "shamir_wide_from_limbs", "shamir_reconstruct_wide",
    "shamir_wide_from_limbs_device", "shamir_reconstruct_wide_checked", "shamir_reconstruct_wide_corrected", "shamir_wide_erasure_mask",
    "shamir_evaluate_wide_corrected",
    "shamir_shares_packed_wide", "deal_party_shares_packed_wide", "shamir_reconstruct_packed_wide", "shamir_reconstruct_packed_wide_corrected",
    "shamir_evaluate_wide_corrected_at", "shamir_packed_wide_secrets",
    "shamir_wide_handover_shape", "shamir_wide_signed_digits", "shamir_wide_handover_weights", "shamir_wide_from_digits",
    "shamir_packed_wide_handover_points", "decrypt_all_party_handover_wide",
    "shamir_handover_weights", "shamir_valid_mask", "decrypt_all_party_handover",
    "device_available", "REPR_POWER", "REPR_NTT",
]

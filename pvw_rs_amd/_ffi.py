"""ctypes declarations for libpvw_hip.so (include/pvw_hip.h).

The product has no CPU fallback: if the library is missing this module raises at
import of the symbols, and every device entry point returns PVW_ERR_INTERNAL
without a gfx950 device."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpvw_hip.so")

PVW_OK = 0
ERROR_NAMES = {
    1: "InvalidParameters", 2: "SamplingError", 3: "EncryptionError", 4: "DecryptionError",
    5: "KeyGenerationError", 6: "CrsError", 7: "SerializationError", 8: "DeserializationError",
    9: "EncodingError", 10: "DecodingError", 11: "ValidationError", 12: "ContextError",
    13: "PolynomialError", 14: "MatrixError", 15: "DimensionMismatch", 16: "IndexOutOfBounds",
    17: "InsufficientData", 18: "InvalidFormat", 19: "InternalError",
}
REPR_POWER, REPR_NTT = 0, 1
RND_SEED, RND_EXPLICIT = 0, 1
DOM_R, DOM_E1, DOM_E2, DOM_SK, DOM_EKEY, DOM_CRS, DOM_GAUSS, DOM_PK, DOM_CALL, DOM_SHAMIR = range(10)
PREPARE_PACKED, PREPARE_MFMA, PREPARE_SUM = 1, 2, 4
WIRE_PARAMS, WIRE_CRS, WIRE_PK, WIRE_CT, WIRE_SK = 1, 2, 3, 4, 5     # wire format v1 kinds


class pvw_params_t(C.Structure):
    _fields_ = [
        ("n", C.c_uint32), ("k", C.c_uint32), ("l", C.c_uint32), ("num_moduli", C.c_uint32),
        ("moduli", C.POINTER(C.c_uint64)), ("secret_variance", C.c_float),
        ("error_bound_1", C.c_uint64), ("error_bound_2", C.c_uint64), ("device", C.c_int32),
        ("party_lo", C.c_uint32), ("party_hi", C.c_uint32), ("c1_lo", C.c_uint32), ("c1_hi", C.c_uint32),
    ]


class pvw_randomness_t(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32), ("seed", C.c_uint8 * 32),
        ("r", C.c_void_p), ("e1", C.c_void_p), ("e2", C.c_void_p),
    ]


_P = C.c_void_p
_SIGNATURES = {
    "pvw_last_error": [C.c_char_p, C.c_size_t],
    "pvw_device_available": [],
    "pvw_ctx_create": [C.POINTER(pvw_params_t), C.POINTER(_P)],
    "pvw_ctx_destroy": [_P],
    "pvw_ctx_get_roots": [_P, _P],
    "pvw_ctx_set_roots": [_P, _P],
    "pvw_ctx_delta": [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)],
    "pvw_ctx_delta_power_l_minus_1": [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)],
    "pvw_ctx_q_total": [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)],
    "pvw_ctx_gadget": [_P, _P, C.c_uint32],
    "pvw_ctx_verify_correctness_condition": [_P, C.POINTER(C.c_int32)],
    "pvw_suggest_error_bounds": [C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_float,
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "pvw_encode_scalar": [_P, C.c_int64, _P, C.c_uint32],
    "pvw_load_crs": [_P, _P, C.c_uint32],
    "pvw_load_crs_device": [_P, _P, C.c_uint32, _P],
    "pvw_crs_generate": [_P, _P],
    "pvw_get_crs": [_P, _P, C.c_uint32],
    "pvw_load_pk": [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32],
    "pvw_load_pk_device": [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P],
    "pvw_pk_fill_uniform": [_P, _P],
    "pvw_get_pk": [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32],
    "pvw_num_public_keys": [_P, C.POINTER(C.c_uint32)],
    "pvw_is_full": [_P, C.POINTER(C.c_int32)],
    "pvw_keygen": [_P, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_sample_secret_keys": [_P, _P, C.c_uint32, C.c_uint32, _P],
    "pvw_keygen_seeded": [_P, C.c_uint32, C.c_uint32, _P, _P],
    "pvw_sample_secret_keys_device": [_P, _P, C.c_uint32, C.c_uint32, _P, _P],
    "pvw_encrypt": [_P, _P, C.c_size_t, C.POINTER(pvw_randomness_t), _P, _P, C.c_uint32],
    "pvw_encrypt_device": [_P, _P, C.c_size_t, C.POINTER(pvw_randomness_t), _P, _P, C.c_uint32, _P],
    "pvw_encrypt_multi": [_P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, C.c_uint32],
    "pvw_encrypt_multi_device": [_P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, C.c_uint32, _P],
    "pvw_rnd_state_create": [_P, _P, C.c_uint64, C.POINTER(_P)],
    "pvw_rnd_state_counter": [_P, _P, C.POINTER(C.c_uint64)],
    "pvw_rnd_state_set_counter": [_P, C.c_uint64, _P],
    "pvw_rnd_state_free": [_P],
    "pvw_rnd_call_seed": [_P, C.c_uint64, _P],
    "pvw_encrypt_rs": [_P, _P, C.c_size_t, _P, _P, _P, C.c_uint32],
    "pvw_encrypt_rs_device": [_P, _P, C.c_size_t, _P, _P, _P, C.c_uint32, _P],
    "pvw_encrypt_multi_rs": [_P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, C.c_uint32],
    "pvw_encrypt_multi_rs_device": [_P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, C.c_uint32, _P],
    "pvw_selftest_rnd_free_residue": [C.POINTER(C.c_uint64)],
    "pvw_decrypt_batch": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P],
    "pvw_decrypt_noisy_device": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P],
    "pvw_decrypt_batch_device": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P],
    "pvw_sk_load": [_P, _P, C.POINTER(C.c_void_p)],
    "pvw_sk_load_seeded": [_P, _P, C.c_uint32, C.POINTER(C.c_void_p)],
    "pvw_sk_free": [_P],
    "pvw_decrypt_batch_device_sk": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P],
    "pvw_decrypt_all": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, C.c_uint32, _P],
    "pvw_decrypt_all_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P],
    "pvw_decrypt_batch_checked": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P],
    "pvw_decrypt_batch_checked_device": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, _P],
    "pvw_decrypt_batch_device_sk_checked": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, _P],
    "pvw_decrypt_all_checked": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P],
    "pvw_decrypt_all_checked_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P],
    "pvw_decode_checked": [_P, _P, C.c_size_t, _P, _P, _P],
    "pvw_decode_checked_device": [_P, _P, C.c_size_t, _P, _P, _P, _P],
    "pvw_decode_checked_host": [_P, _P, C.c_size_t, _P, _P, _P],
    "pvw_selftest_decode_checked": [_P, _P, C.c_size_t, _P, _P, _P],
    "pvw_ctx_noise_bound": [_P, C.POINTER(C.c_uint64)],
    "pvw_ct_sum_device": [_P, _P, _P, C.c_size_t, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P],
    "pvw_ct_sum": [_P, _P, _P, C.c_size_t, _P, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_ct_sum_host": [_P, _P, _P, C.c_size_t, _P, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_decrypt_sum_checked_device": [_P, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, _P, _P],
    "pvw_decrypt_sum_device_sk_checked": [_P, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, _P, _P],
    "pvw_decrypt_sum_checked": [_P, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P],
    "pvw_decrypt_all_sum_checked": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P],
    "pvw_decrypt_all_sum_checked_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, _P],
    "pvw_ctx_sum_capacity": [_P, C.POINTER(C.c_uint64)],
    "pvw_ct_lincomb_device": [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P],
    "pvw_ct_lincomb": [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_ct_lincomb_host": [_P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_decrypt_lincomb_plain": [_P, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_lincomb_plain_device": [_P, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_lincomb_device_sk_plain": [_P, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_all_lincomb_plain": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_all_lincomb_plain_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_ctx_lincomb_fits": [_P, _P, C.c_size_t, _P, C.POINTER(C.c_uint32)],
    "pvw_shamir_lagrange_weights": [C.c_uint64, _P, C.c_size_t, _P],
    "pvw_shamir_lagrange_weights_at": [C.c_uint64, _P, C.c_size_t, _P, C.c_size_t, _P],
    "pvw_ct_lincomb_many_host": [_P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_ct_lincomb_many_device": [_P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P, _P, _P],
    "pvw_ct_lincomb_many": [_P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P, _P],
    "pvw_decrypt_all_lincomb_many_plain_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_all_lincomb_many_plain": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    # one-word handover from a mask: the weights [T][D], the mask from a report, the handover in one call
    "pvw_shamir_handover_weights_host": [C.c_uint64, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P],
    "pvw_shamir_handover_weights_device": [_P, C.c_uint64, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P],
    "pvw_shamir_valid_mask_host": [_P, _P, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P],
    "pvw_shamir_valid_mask_device": [_P, _P, _P, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P],
    "pvw_decrypt_all_handover_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P,
                                        C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_all_handover": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P,
                                 C.c_uint64, C.c_uint32, _P],
    # plain-modulus decode: the checked call plus (plain_modulus, wide_words, wide)
    "pvw_decode_plain": [_P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decode_plain_device": [_P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decode_plain_host": [_P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_selftest_decode_plain": [_P, _P, C.c_size_t, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_batch_plain": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_batch_plain_device": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_batch_device_sk_plain": [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_all_plain": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_all_plain_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_sum_plain": [_P, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_sum_plain_device": [_P, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_sum_device_sk_plain": [_P, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    "pvw_decrypt_all_sum_plain": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P],
    "pvw_decrypt_all_sum_plain_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P],
    # Shamir shares
    "pvw_shamir_shares_host": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P],
    "pvw_shamir_shares_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P, _P],
    "pvw_shamir_shares": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P],
    "pvw_deal_shares": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32, _P],
    "pvw_deal_shares_rs": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_rs_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32, _P],
    "pvw_shamir_reconstruct": [C.c_uint64, _P, _P, C.c_size_t, C.c_size_t, _P],
    # packed sharing: the 8.9 calls with `pack` after num_dealers; reconstruct (p, pack, indices, shares, count, rows, out)
    # Shamir shares over a prime below 2^256: plain_modulus is a pointer to four words
    "pvw_shamir_wide_limbs": [_P, C.c_uint32, _P],
    "pvw_shamir_shares_wide_host": [_P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P],
    "pvw_shamir_shares_wide_device": [_P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, _P],
    "pvw_shamir_shares_wide": [_P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P],
    "pvw_deal_shares_wide": [_P, _P, C.c_size_t, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_wide_device": [_P, _P, C.c_size_t, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P],
    "pvw_deal_shares_wide_rs": [_P, _P, C.c_size_t, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_wide_rs_device": [_P, _P, C.c_size_t, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P],
    "pvw_shamir_wide_to_limbs_host": [_P, C.c_size_t, C.c_uint32, C.c_uint32, _P],
    "pvw_shamir_wide_from_limbs_host": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P],
    "pvw_shamir_reconstruct_wide": [_P, _P, _P, C.c_size_t, C.c_size_t, _P],
    "pvw_selftest_shamir_wide_step": [_P, _P, _P, _P, _P, C.c_size_t, _P],
    # packed sharing over a prime below 2^256: the 8.18 calls with `pack` after num_dealers
    "pvw_shamir_shares_packed_wide_host": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P, _P, _P],
    "pvw_shamir_shares_packed_wide_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P],
    "pvw_shamir_shares_packed_wide": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P, _P, _P],
    "pvw_deal_shares_packed_wide": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_packed_wide_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P],
    "pvw_deal_shares_packed_wide_rs": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_packed_wide_rs_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P],
    "pvw_shamir_reconstruct_packed_wide": [_P, C.c_uint32, _P, _P, C.c_size_t, C.c_size_t, _P],
    "pvw_shamir_wide_from_limbs_device": [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P],
    "pvw_shamir_reconstruct_wide_checked_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P],
    "pvw_shamir_reconstruct_wide_checked_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_wide_checked": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P],
    "pvw_shamir_reconstruct_wide_corrected_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_wide_corrected_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P,
                                                     _P],
    "pvw_shamir_reconstruct_wide_corrected": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P],
    # wide reconstruction with erasures: the wide corrected calls with `erased` directly behind point_stride
    "pvw_shamir_reconstruct_wide_erasures_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P,
                                                  _P],
    "pvw_shamir_reconstruct_wide_erasures_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P,
                                                    _P, _P, _P],
    "pvw_shamir_reconstruct_wide_erasures": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P,
                                             _P],
    # wide share repair: the wide corrected / erasures arguments, then targets, num_targets, values and the four outputs
    "pvw_shamir_evaluate_wide_corrected_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P,
                                                _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_corrected_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P,
                                                  C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_corrected": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P,
                                           _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_erasures_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t,
                                               _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_erasures_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P,
                                                 C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_erasures": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t,
                                          _P, _P, _P, _P, _P],
    "pvw_shamir_wide_erasure_mask_host": [_P, _P, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32,
                                          C.c_size_t, _P],
    "pvw_shamir_wide_erasure_mask_device": [_P, _P, _P, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                            C.c_uint32, C.c_size_t, _P, _P],
    "pvw_selftest_shamir_wide_mul": [_P, _P, _P, _P, C.c_size_t, _P],
    # wide handover: the weight rows of one many-combinations pass and the fold of its digit plaintexts
    "pvw_shamir_wide_handover_shape": [_P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "pvw_shamir_wide_signed_digits_host": [_P, _P, C.c_size_t, C.c_uint32, _P],
    "pvw_shamir_wide_signed_digits_device": [_P, _P, _P, C.c_size_t, C.c_uint32, _P, _P],
    "pvw_shamir_wide_handover_weights_host": [_P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P],
    "pvw_shamir_wide_handover_weights_device": [_P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P, _P],
    "pvw_shamir_wide_from_digits_host": [_P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint32, C.c_size_t, _P, _P],
    "pvw_shamir_wide_from_digits_device": [_P, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint32, C.c_size_t, _P, _P, _P],
    "pvw_decrypt_all_handover_wide": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t,
                                      C.c_uint32, _P, _P, _P],
    "pvw_decrypt_all_handover_wide_device": [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P, C.c_uint32, C.c_uint32, _P, _P, _P,
                                             C.c_size_t, C.c_uint32, _P, _P, _P, _P],
    "pvw_ctx_wide_handover_fits": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)],
    # wide share repair at field points: the 8.22 calls with points [T][4], num_points for targets, num_targets; and
    # the packed secrets (p, pack, degree, indices, count, shares, rows, strides, erased, secrets, nerr, col_err, err_mask)
    "pvw_shamir_evaluate_wide_corrected_at_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t,
                                                   _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_corrected_at_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P,
                                                     C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_corrected_at": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t,
                                              _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_erasures_at_host": [_P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P,
                                                  C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_erasures_at_device": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P,
                                                    C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_wide_erasures_at": [_P, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P,
                                             C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_packed_wide_secrets_host": [_P, C.c_uint32, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P,
                                            _P, _P, _P],
    "pvw_shamir_packed_wide_secrets_device": [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P,
                                              _P, _P, _P, _P, _P],
    "pvw_shamir_packed_wide_secrets": [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P,
                                       _P, _P, _P],
    "pvw_shamir_shares_packed_host": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P],
    "pvw_shamir_shares_packed_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P, _P],
    "pvw_shamir_shares_packed": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P],
    "pvw_deal_shares_packed": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_packed_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32, _P],
    "pvw_deal_shares_packed_rs": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32],
    "pvw_deal_shares_packed_rs_device": [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_uint32, _P],
    "pvw_shamir_reconstruct_packed": [C.c_uint64, C.c_uint32, _P, _P, C.c_size_t, C.c_size_t, _P],
    # checked reconstruction: (p, degree, indices, count, shares, S, secret_stride, point_stride, out, bad, col_bad)
    "pvw_shamir_reconstruct_checked_host": [C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P],
    "pvw_shamir_reconstruct_checked_device": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_checked": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P],
    "pvw_shamir_reconstruct_corrected_host": [C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_corrected_device": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_corrected": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P],
    "pvw_shamir_evaluate_corrected_host": [C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_corrected_device": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_corrected": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, _P],
    # reconstruction with erasures: the corrected / evaluate arguments with `erased` behind point_stride
    "pvw_shamir_reconstruct_erasures_host": [C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_erasures_device": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_reconstruct_erasures": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_erasures_host": [C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_erasures_device": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P],
    "pvw_shamir_evaluate_erasures": [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P, _P, _P, _P, _P],
    "pvw_shamir_erasure_mask_host": [_P, _P, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P],
    "pvw_shamir_erasure_mask_device": [_P, _P, _P, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P],
    "pvw_decode": [_P, _P, C.c_size_t, _P],
    "pvw_decode_host": [_P, _P, C.c_size_t, _P],
    "pvw_decode_device": [_P, _P, C.c_size_t, _P, _P],
    "pvw_selftest_decode_fixed": [_P, _P, C.c_size_t, _P],
    "pvw_selftest_mfma_i8": [_P, _P, _P, _P],
    "pvw_selftest_secret_residue": [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "pvw_selftest_siphash": [_P, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)],
    "pvw_selftest_decode_tables": [_P, C.POINTER(C.c_uint32)],
    "pvw_selftest_decode_shortcuts": [_P, _P, C.c_size_t, _P, _P],
    "pvw_build_is_tuning": [],
    "pvw_crs_seed_from_tag": [C.c_char_p, _P],
    "pvw_ntt_forward": [_P, _P, C.c_size_t],
    "pvw_ntt_inverse": [_P, _P, C.c_size_t],
    "pvw_small_to_poly": [_P, _P, C.c_size_t, _P, C.c_uint32],
    "pvw_sample_cbd": [_P, _P, C.c_uint32, C.c_uint32, C.c_size_t, C.c_float, _P],
    "pvw_sample_uniform": [_P, _P, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint64, _P],
    "pvw_sample_gaussian": [_P, _P, C.c_uint32, C.c_size_t, C.c_uint64, _P],
    "pvw_ctx_set_profiling": [_P, C.c_int32],
    "pvw_ctx_kernel_time": [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)],
    "pvw_ctx_reset_profiling": [_P],
    "pvw_host_alloc": [C.c_size_t, C.POINTER(_P)],
    "pvw_host_free": [_P],
    "pvw_ctx_resident_bytes": [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "pvw_ctx_derived_bytes": [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "pvw_prepare": [_P, C.c_uint32, _P, C.POINTER(C.c_uint64)],
    "pvw_ctx_packed_active": [_P, C.POINTER(C.c_uint32)],
    "pvw_ctx_synchronize": [_P],
    "pvw_wire_poly_bytes": [_P, C.POINTER(C.c_size_t)],
    "pvw_wire_header": [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_size_t,
                        C.POINTER(C.c_size_t)],
    "pvw_wire_header_check": [_P, _P, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P, C.POINTER(C.c_size_t)],
    "pvw_wire_pack": [_P, _P, C.c_size_t, _P],
    "pvw_wire_pack_device": [_P, _P, C.c_size_t, _P, _P],
    "pvw_wire_unpack": [_P, _P, C.c_size_t, _P],
    "pvw_wire_unpack_device": [_P, _P, C.c_size_t, _P, _P, _P],
    "pvw_wire_pack_host": [_P, _P, C.c_size_t, _P],
    "pvw_wire_unpack_host": [_P, _P, C.c_size_t, _P, C.POINTER(C.c_uint64)],
    "pvw_load_pk_wire": [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32],
    "pvw_get_pk_wire": [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32],
    "pvw_load_crs_wire": [_P, _P, C.c_uint32],
    "pvw_get_crs_wire": [_P, _P, C.c_uint32],
}

# include/pvw_hip_tuning.h: exported by the measurement build only
_TUNING_SIGNATURES = {
    "pvw_selftest_read_bandwidth": [_P, C.c_uint32, _P, _P],
    "pvw_tuning_read_stamps": [_P, _P, _P, C.c_uint32],
    "pvw_tuning_read_probe": [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P],
}

LIB_TUNING_PATH = os.path.join(HERE, "libpvw_hip_tuning.so")
_libs = {}
# which build `lib()` hands out: always the shipped library unless CODE asks for the measurement build with
# `select("tuning")` (tools/*.py, bench.py --tuning-library, tests/test_gpu_tuning.py).  Nothing in the environment can
# redirect the package to it -- that build honours switches that change what encrypt computes.  Every PvwParameters
# remembers the library it was created with.
_selected = "default"


def _load(which: str) -> C.CDLL:
    if which not in _libs:
        path = LIB_TUNING_PATH if which == "tuning" else LIB_PATH
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: the PVW hot path is HIP-only, run "
                "`python -c 'import __graft_entry__ as g; g.build()'` first")
        L = C.CDLL(path)
        sigs = dict(_SIGNATURES)
        if which == "tuning":
            sigs.update(_TUNING_SIGNATURES)
        for name, args in sigs.items():
            fn = getattr(L, name)          # AttributeError if the library lacks a declared symbol
            fn.argtypes = args
            fn.restype = C.c_int32
        _libs[which] = L
    return _libs[which]


def lib() -> C.CDLL:
    """The selected HIP library (libpvw_hip.so unless the tuning build was selected)."""
    return _load(_selected)


def tuning_lib() -> C.CDLL:
    """libpvw_hip_tuning.so (-DPVW_TUNING=1): schedule selectors, timing ablations, bandwidth probe."""
    return _load("tuning")


def select(which: str) -> str:
    """Choose the build later `lib()` calls return ("default" | "tuning"); returns the previous choice."""
    global _selected
    if which not in ("default", "tuning"):
        raise ValueError(which)
    prev, _selected = _selected, which
    return prev


def last_error(L: C.CDLL = None) -> str:
    buf = C.create_string_buffer(512)
    (L or lib()).pvw_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")

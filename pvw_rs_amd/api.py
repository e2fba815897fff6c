"""Host-side mirror of `pvw::{params, crs, keys, crypto}` over the C ABI (include/pvw_hip.h).

Same names, argument meaning and error behaviour as the reference's Rust API so that the
parity tests read like the reference's own tests (tests/crypto.rs, tests/params.rs,
tests/keys.rs).  Everything heavy happens in libpvw_hip.so on the GPU; this file only
marshals numpy arrays.  Differences forced by the boundary:

  * randomness is an explicit input (a 32-byte seed or explicit small polynomials): the
    reference draws from thread_rng() (src/crypto/encryption.rs:138,164,180);
  * one PvwParameters object owns one device context, which holds at most one CRS and one
    GlobalPublicKey (the device-resident A-hat / B-hat);
  * polynomials are numpy arrays [L][l] uint64 (power basis unless stated otherwise).
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import REPR_NTT, REPR_POWER


class PvwError(Exception):
    """PvwError (src/errors.rs:13-70): `.variant` is the Rust variant name."""

    def __init__(self, code: int, message: str):
        self.code = code
        self.variant = _ffi.ERROR_NAMES.get(code, f"Unknown({code})")
        super().__init__(f"{self.variant}: {message}")


def _check(rc: int, lib=None) -> None:
    if rc != _ffi.PVW_OK:
        raise PvwError(rc, _ffi.last_error(lib))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def _i64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64)


def _seed(seed: bytes) -> np.ndarray:
    if len(seed) != 32:
        raise PvwError(1, "seed must be 32 bytes")
    return np.frombuffer(bytes(seed), dtype=np.uint8).copy()


def device_available() -> bool:
    return bool(_ffi.lib().pvw_device_available())


# ------------------------------------------------------------------------------------
# params (src/params/parameters.rs)
# ------------------------------------------------------------------------------------
class PvwParametersBuilder:
    """parameters.rs:44-201."""

    def __init__(self):
        self._n = self._k = self._l = self._moduli = None
        self._variance = self._b1 = self._b2 = None
        self._device = -1
        self._shard = (0, 0, 0, 0)

    @staticmethod
    def new() -> "PvwParametersBuilder":
        return PvwParametersBuilder()

    def set_parties(self, n): self._n = n; return self
    def set_dimension(self, k): self._k = k; return self
    def set_l(self, l): self._l = l; return self
    def set_moduli(self, moduli): self._moduli = list(moduli); return self
    def set_secret_variance(self, v): self._variance = float(v); return self
    def set_error_bound_1(self, b): self._b1 = int(b); return self
    def set_error_bound_2(self, b): self._b2 = int(b); return self
    def set_error_bounds(self, b1, b2): self._b1, self._b2 = int(b1), int(b2); return self
    def set_error_bounds_u32(self, b1, b2): return self.set_error_bounds(b1, b2)

    # not in the reference: device placement and the party shard of a multi-GPU job
    def set_device(self, ordinal): self._device = int(ordinal); return self

    def set_shard(self, party_lo, party_hi, c1_lo, c1_hi):
        self._shard = (party_lo, party_hi, c1_lo, c1_hi)
        return self

    def build(self) -> "PvwParameters":
        for name, v in (("n", self._n), ("k", self._k), ("l", self._l), ("moduli", self._moduli)):
            if v is None:
                raise PvwError(1, f"{name} not set")                      # parameters.rs:118-129
        b1 = 100 if self._b1 is None else self._b1                        # :167
        b2 = 200 if self._b2 is None else self._b2                        # :168
        if b1 <= 0:
            raise PvwError(1, "error_bound_1 must be positive")          # :172
        if b2 <= 0:
            raise PvwError(1, "error_bound_2 must be positive")          # :177
        if b1 >= 1 << 62 or b2 >= 1 << 62:
            raise PvwError(1, "error bounds must be below 2^62")
        variance = 0.5 if self._variance is None else self._variance     # :166
        return PvwParameters(self._n, self._k, self._l, self._moduli, variance, b1, b2,
                             self._device, self._shard)

    build_arc = build


class PvwParameters:
    """PvwParameters (parameters.rs:19-40) + the device context behind it."""

    def __init__(self, n, k, l, moduli, secret_variance, error_bound_1, error_bound_2,
                 device=-1, shard=(0, 0, 0, 0)):
        for name, v in (("n", n), ("k", k), ("l", l)):
            if not (0 <= int(v) < 1 << 32):
                raise PvwError(1, f"{name} out of range")
        self.n, self.k, self.l = int(n), int(k), int(l)
        self._moduli = _u64(list(moduli))
        self.secret_variance = float(secret_variance)
        self.error_bound_1, self.error_bound_2 = int(error_bound_1), int(error_bound_2)
        p = _ffi.pvw_params_t()
        p.n, p.k, p.l, p.num_moduli = self.n, self.k, self.l, len(self._moduli)
        p.moduli = self._moduli.ctypes.data_as(C.POINTER(C.c_uint64))
        p.secret_variance = self.secret_variance
        p.error_bound_1, p.error_bound_2 = self.error_bound_1, self.error_bound_2
        p.device = device
        p.party_lo, p.party_hi, p.c1_lo, p.c1_hi = shard
        h = C.c_void_p()
        self._h = None
        self._lib = _ffi.lib()              # the build selected now serves this context for its whole life
        _check(self._lib.pvw_ctx_create(C.byref(p), C.byref(h)), self._lib)
        self._h = h
        self.t = (self.n - 1) // 2                                        # :169
        self.party_lo, self.party_hi = (shard[0], shard[1]) if (shard[0] or shard[1]) else (0, self.n)
        self.c1_lo, self.c1_hi = (shard[2], shard[3]) if (shard[2] or shard[3]) else (0, self.k)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                self._lib.pvw_ctx_destroy(self._h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def builder() -> PvwParametersBuilder:
        return PvwParametersBuilder()

    @staticmethod
    def new_with_u32_bounds(n, k, l, moduli, variance, b1, b2) -> "PvwParameters":   # :231-249
        return (PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
                .set_secret_variance(variance).set_error_bounds_u32(b1, b2).build())

    # -- accessors -----------------------------------------------------------------
    @property
    def L(self) -> int:
        return len(self._moduli)

    def moduli(self) -> List[int]:
        return [int(q) for q in self._moduli]

    def _call(self, name: str, *args) -> None:
        """one C-ABI call on this context, through the library the context was created with"""
        rc = getattr(self._lib, name)(self._h, *args)
        if rc != _ffi.PVW_OK:
            raise PvwError(rc, _ffi.last_error(self._lib))

    def _big(self, name) -> int:
        n = C.c_size_t()
        self._call(name, None, 0, C.byref(n))
        w = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._call(name, _ptr(w), len(w), C.byref(n))
        return sum(int(w[i]) << (64 * i) for i in range(n.value))

    def delta(self) -> int:
        return self._big("pvw_ctx_delta")

    def delta_power_l_minus_1(self) -> int:
        return self._big("pvw_ctx_delta_power_l_minus_1")

    def q_total(self) -> int:
        return self._big("pvw_ctx_q_total")

    def roots(self) -> List[int]:
        w = np.zeros(self.L, dtype=np.uint64)
        self._call("pvw_ctx_get_roots", _ptr(w))
        return [int(x) for x in w]

    def set_roots(self, psi: Sequence[int]) -> None:
        w = _u64(list(psi))
        if len(w) != self.L:
            raise PvwError(15, f"expected {self.L}, got {len(w)}")
        self._call("pvw_ctx_set_roots", _ptr(w))

    def gadget_polynomial(self, repr: int = REPR_POWER) -> np.ndarray:   # :288-308
        out = np.zeros((self.L, self.l), dtype=np.uint64)
        self._call("pvw_ctx_gadget", _ptr(out), repr)
        return out

    def gadget_vector(self) -> List[int]:                                 # :311-324
        d = self.delta()
        return [d ** j for j in range(self.l)]

    def encode_scalar(self, scalar: int, repr: int = REPR_POWER) -> np.ndarray:   # :346-367
        out = np.zeros((self.L, self.l), dtype=np.uint64)
        self._call("pvw_encode_scalar", C.c_int64(scalar), _ptr(out), repr)
        return out

    def verify_correctness_condition(self) -> bool:                       # :510-551
        ok = C.c_int32()
        self._call("pvw_ctx_verify_correctness_condition", C.byref(ok))
        return bool(ok.value)

    def noise_bound(self) -> int:
        """total_bound of verify_correctness_condition (parameters.rs:516-543), floored and saturated to u64: the default
        bound a checked decrypt's noise is held to."""
        v = C.c_uint64()
        self._call("pvw_ctx_noise_bound", C.byref(v))
        return int(v.value)

    def sum_capacity(self) -> int:
        """pvw_ctx_sum_capacity: the number of dealers' ciphertexts, each at noise_bound(), whose sum is PROVEN to decode exactly
        (floor(R / noise_bound()), R (Delta^(l-1) + 1) < Q / 2).  Advisory and sufficient only: honest noise is far below
        noise_bound(), and the checked decode of an aggregate reports its exact noise."""
        v = C.c_uint64()
        self._call("pvw_ctx_sum_capacity", C.byref(v))
        return int(v.value)

    def lincomb_fits(self, weights, valid=None) -> bool:
        """pvw_ctx_lincomb_fits: whether (sum of |w_d| over the participating dealers -- valid and weight not 0) * noise_bound()
        stays inside the radius sum_capacity() is built on, so that the decode of the combination is PROVEN exact.  Advisory
        and sufficient only, like sum_capacity()."""
        w = np.ascontiguousarray(np.array([int(x) for x in weights], dtype=np.int64))
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        if v is not None and v.shape != w.shape:
            raise PvwError(15, f"valid: expected {w.size} flags, got {v.size}")
        fits = C.c_uint32()
        self._call("pvw_ctx_lincomb_fits", _ptr(w), w.size, _ptr(v), C.byref(fits))
        return bool(fits.value)

    def wide_handover_fits(self, plain_modulus: int, num_valid: int, limb_bits: int = 52, digit_bits: int = 64) -> bool:
        """pvw_ctx_wide_handover_fits: lincomb_fits for every weight row of a wide handover at once -- num_valid * NL
        weights of at most 2^(digit_bits - 1) each -- and the digit plaintexts fit the words of Q.  Advisory and sufficient only."""
        fits = C.c_uint32()
        self._call("pvw_ctx_wide_handover_fits", _ptr(_wide_modulus(plain_modulus)), int(num_valid), int(limb_bits), int(digit_bits),
                   C.byref(fits))
        return bool(fits.value)

    @staticmethod
    def suggest_error_bounds(n, k, l, moduli, variance) -> Tuple[int, int]:   # :554-603
        m = _u64(list(moduli))
        b1, b2 = C.c_uint32(), C.c_uint32()
        _check(_ffi.lib().pvw_suggest_error_bounds(n, k, l, _ptr(m), len(m), variance,
                                                   C.byref(b1), C.byref(b2)))
        return b1.value, b2.value

    # -- ring primitives (fhe-math call sites) ----------------------------------------
    def bigints_to_poly(self, bigints: Sequence[int]) -> np.ndarray:     # :420-474 (host marshalling)
        if len(bigints) != self.l:
            raise PvwError(1, f"Expected {self.l} coefficients, got {len(bigints)}")
        return np.array([[int(c) % int(q) for c in bigints] for q in self._moduli], dtype=np.uint64)

    def poly_to_bigints(self, poly: np.ndarray) -> List[int]:
        """Vec<BigUint>::from(&Poly): CRT lift to [0, Q)."""
        Q = self.q_total()
        out = [0] * self.l
        for i, q in enumerate(self.moduli()):
            Qi = Q // q
            inv = pow(Qi, -1, q)
            for c in range(self.l):
                out[c] = (out[c] + int(poly[i, c]) * inv % q * Qi) % Q
        return out

    def from_coefficients(self, coeffs, repr: int = REPR_NTT) -> np.ndarray:
        """Poly::from_coefficients(&[i64]) (+ change_representation(Ntt)) on the device."""
        a = _i64(coeffs)
        count = a.size // self.l
        out = np.zeros(a.shape[:-1] + (self.L, self.l), dtype=np.uint64)
        self._call("pvw_small_to_poly", _ptr(a), count, _ptr(out), repr)
        return out

    def ntt_forward(self, polys) -> np.ndarray:
        a = _u64(polys).copy()
        self._call("pvw_ntt_forward", _ptr(a), a.size // (self.L * self.l))
        return a

    def ntt_inverse(self, polys) -> np.ndarray:
        a = _u64(polys).copy()
        self._call("pvw_ntt_inverse", _ptr(a), a.size // (self.L * self.l))
        return a

    # -- samplers (src/sampling) --------------------------------------------------------
    def sample_vec_cbd(self, seed: bytes, domain: int, index0: int, count: int, variance=None) -> np.ndarray:
        out = np.zeros((count, self.l), dtype=np.int64)
        v = self.secret_variance if variance is None else variance
        self._call("pvw_sample_cbd", _ptr(_seed(seed)), domain, index0, count, v, _ptr(out))
        return out

    def sample_uniform_coefficients(self, seed: bytes, domain: int, index0: int, count: int, bound: int) -> np.ndarray:
        out = np.zeros((count, self.l), dtype=np.int64)
        self._call("pvw_sample_uniform", _ptr(_seed(seed)), domain, index0, count, bound, _ptr(out))
        return out

    def sample_discrete_gaussian_vec(self, seed: bytes, bound: int, n: int, index0: int = 0) -> np.ndarray:
        out = np.zeros(n, dtype=np.int64)
        self._call("pvw_sample_gaussian", _ptr(_seed(seed)), index0, n, bound, _ptr(out))
        return out

    # -- measurement ----------------------------------------------------------------------
    def set_profiling(self, on: bool) -> None:
        self._call("pvw_ctx_set_profiling", int(on))

    def reset_profiling(self) -> None:
        self._call("pvw_ctx_reset_profiling")

    def kernel_time(self, name: str) -> Tuple[float, int]:
        ms, cnt = C.c_double(), C.c_uint64()
        self._call("pvw_ctx_kernel_time", name.encode(), C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value

    def resident_bytes(self) -> Tuple[int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        self._call("pvw_ctx_resident_bytes", C.byref(a), C.byref(b))
        return a.value, b.value

    def prepare(self, flags: int = _ffi.PREPARE_PACKED | _ffi.PREPARE_MFMA, stream=None) -> int:
        """pvw_prepare: build the derived copies of the resident matrices (and `stream`'s workspace) now; returns the
        bytes allocated for them.  After it, *_device calls on that stream neither allocate nor synchronise."""
        taken = C.c_uint64(0)
        self._call("pvw_prepare", int(flags), C.c_void_p(stream) if stream else None, C.byref(taken))
        return int(taken.value)

    def packed_active(self) -> int:
        """bits per residue of the packed stream single-dealer encrypt would use right now (0 = the tiled matrices)"""
        w = C.c_uint32(0)
        self._call("pvw_ctx_packed_active", C.byref(w))
        return int(w.value)

    def derived_bytes(self) -> Tuple[int, int]:
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._call("pvw_ctx_derived_bytes", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def synchronize(self) -> None:
        self._call("pvw_ctx_synchronize")

    # -- wire format v1 ----------------------------------------------------------
    def wire_poly_bytes(self) -> int:
        """bytes of one packed polynomial: (l/8) * sum_i bitlen(q_i)"""
        out = C.c_size_t()
        self._call("pvw_wire_poly_bytes", C.byref(out))
        return int(out.value)

    def to_bytes(self) -> bytes:
        """the parameters as a wire blob of kind 1 (a header, no body)"""
        return bytes(_wire_header(self, _ffi.WIRE_PARAMS))

    @staticmethod
    def from_bytes(data, device: int = -1) -> "PvwParameters":
        """parameters from a kind-1 blob (host only: no device work)"""
        raw = bytes(data[:_WIRE_FIXED]) if len(data) >= _WIRE_FIXED else b""
        if len(raw) < _WIRE_FIXED or raw[:4] != _WIRE_MAGIC:
            raise PvwError(18, "wire: truncated header or bad magic")
        version, kind = struct.unpack_from("<HH", raw, 4)
        if version != 1 or kind != _ffi.WIRE_PARAMS:
            raise PvwError(18, f"wire: version {version} kind {kind}, expected version 1 kind {_ffi.WIRE_PARAMS}")
        n, k, l, L, var, b1, b2 = struct.unpack_from("<IIIIfQQ", raw, 12)
        if len(data) < _WIRE_FIXED + 8 * L:
            raise PvwError(18, "wire: truncated header")
        moduli = list(struct.unpack_from(f"<{L}Q", bytes(data[_WIRE_FIXED:_WIRE_FIXED + 8 * L])))
        p = PvwParameters(n, k, l, moduli, var, b1, b2, device)
        _wire_check(p, data, _ffi.WIRE_PARAMS)
        return p


# ------------------------------------------------------------------------------------
# CRS (src/params/crs.rs)
# ------------------------------------------------------------------------------------
class PvwCrs:
    """PvwCrs (crs.rs:12-17): the k x k matrix lives on the device of `params`."""

    def __init__(self, params: PvwParameters):
        self.params = params

    @staticmethod
    def new(params: PvwParameters, rng=None) -> "PvwCrs":                    # crs.rs:24-39
        """Fresh random CRS: `rng` is anything with `.bytes(32)` / `.randbytes(32)` (default: the OS entropy
        source, the reference takes a CryptoRng); the polynomials come from this library's seeded streams."""
        if rng is None:
            import os
            seed = os.urandom(32)
        else:
            seed = bytes(rng.bytes(32) if hasattr(rng, "bytes") else rng.randbytes(32))
        return PvwCrs.new_deterministic(params, seed)

    @staticmethod
    def seed_from_tag(tag: str) -> bytes:
        """The 32-byte seed PvwCrs::new_from_tag derives (crs.rs:75-87): DefaultHasher(tag + "CRS") as 8
        little-endian bytes, repeated four times."""
        out = np.zeros(32, dtype=np.uint8)
        _check(_ffi.lib().pvw_crs_seed_from_tag(tag.encode("utf-8"), _ptr(out)))
        return out.tobytes()

    @staticmethod
    def new_from_tag(params: PvwParameters, tag: str) -> "PvwCrs":           # crs.rs:74-90
        return PvwCrs.new_deterministic(params, PvwCrs.seed_from_tag(tag))

    @staticmethod
    def new_deterministic(params: PvwParameters, seed: bytes) -> "PvwCrs":   # crs.rs:45-67
        params._call("pvw_crs_generate", _ptr(_seed(seed)))
        return PvwCrs(params)

    @staticmethod
    def from_polynomials(params: PvwParameters, a: np.ndarray, repr: int = REPR_POWER) -> "PvwCrs":
        a = _u64(a)
        want = (params.k, params.k, params.L, params.l)
        if a.shape != want:
            raise PvwError(15, f"expected {want}, got {a.shape}")
        params._call("pvw_load_crs", _ptr(a), repr)
        return PvwCrs(params)

    def dimensions(self) -> Tuple[int, int]:
        return self.params.k, self.params.k

    def matrix(self, repr: int = REPR_POWER) -> np.ndarray:
        p = self.params
        out = np.zeros((p.k, p.k, p.L, p.l), dtype=np.uint64)
        p._call("pvw_get_crs", _ptr(out), repr)
        return out

    def get(self, i: int, j: int, repr: int = REPR_POWER) -> Optional[np.ndarray]:   # crs.rs:93
        if not (0 <= i < self.params.k and 0 <= j < self.params.k):
            return None
        return self.matrix(repr)[i, j]

    def validate(self) -> None:
        return None

    def to_bytes(self, repr: int = REPR_POWER) -> bytes:
        """the rows this context holds as a wire blob of kind 2 (packed on the device)"""
        p = self.params
        pb = p.wire_poly_bytes() * p.k
        full = np.zeros(p.k * pb, dtype=np.uint8)
        p._call("pvw_get_crs_wire", _ptr(full), repr)
        return bytes(_wire_header(p, _ffi.WIRE_CRS, repr, p.c1_lo, p.c1_hi)) + full[p.c1_lo * pb:p.c1_hi * pb].tobytes()

    @staticmethod
    def from_bytes(params: PvwParameters, data) -> "PvwCrs":
        """load a kind-2 blob (checked on the device: a residue >= q_i raises DeserializationError, nothing is loaded)"""
        repr, rg, hl, a = _wire_check(params, data, _ffi.WIRE_CRS)
        if not (rg[0] <= params.c1_lo and params.c1_hi <= rg[1]):
            raise PvwError(18, f"wire: the blob holds CRS rows [{rg[0]}, {rg[1]}), this context needs [{params.c1_lo}, {params.c1_hi})")
        pb = params.wire_poly_bytes() * params.k
        full = np.zeros(params.k * pb + 1, dtype=np.uint8)
        full[rg[0] * pb:rg[1] * pb] = a[hl:]
        params._call("pvw_load_crs_wire", _ptr(full), repr)
        return PvwCrs(params)


# ------------------------------------------------------------------------------------
# keys (src/keys)
# ------------------------------------------------------------------------------------
class SecretKey:
    """SecretKey (secret_key.rs:14-18): k x l CBD coefficients."""

    def __init__(self, params: PvwParameters, secret_coeffs: np.ndarray):
        self.params = params
        self.secret_coeffs = np.array(secret_coeffs, dtype=np.int64, order="C", copy=True)   # owned: zeroized on drop

    @staticmethod
    def random(params: PvwParameters, seed: bytes, party_index: int = 0) -> "SecretKey":   # :45-63
        out = np.zeros((params.k, params.l), dtype=np.int64)
        params._call("pvw_sample_secret_keys", _ptr(_seed(seed)), party_index, 1, _ptr(out))
        key = SecretKey(params, out)
        out.fill(0)
        return key

    @staticmethod
    def from_coefficients(params: PvwParameters, coeffs) -> "SecretKey":
        a = _i64(coeffs)
        if a.shape != (params.k, params.l):
            raise PvwError(1, f"Secret key has shape {a.shape} but expected {(params.k, params.l)}")
        return SecretKey(params, a)

    def coefficients(self) -> np.ndarray:
        """A COPY of the coefficients (secret_key.rs:280-292 hands out a slice tied to the key's lifetime; numpy cannot
        express that, and a view would silently turn to zeros when the key is dropped).  The caller owns the copy and
        wipes it.  `secret_coeffs` is the key's own storage: cleared by zeroize() / on drop."""
        return self.secret_coeffs.copy()

    def zeroize(self) -> None:
        """Zeroize / ZeroizeOnDrop (secret_key.rs:20-30): overwrite the coefficients in place (the device side
        clears its own copies before every call returns, see pvw_selftest_secret_residue)."""
        if getattr(self, "secret_coeffs", None) is not None and self.secret_coeffs.flags.writeable:
            self.secret_coeffs.fill(0)

    def __del__(self):
        try:
            self.zeroize()
        except Exception:
            pass

    def load_device(self) -> "DeviceSecretKey":
        """The key in the form the inner products of decrypt read (NTT(sk[j]), secret_key.rs:98-112), resident on the
        device until the returned handle is freed: pvw_decrypt_batch_device_sk then neither transforms nor wipes per call."""
        return DeviceSecretKey(self)

    def get_polynomial(self, index: int) -> np.ndarray:                   # :98-112 (NTT form)
        if not 0 <= index < len(self.secret_coeffs):
            raise PvwError(1, f"Index {index} out of bounds for {len(self.secret_coeffs)} polynomials")
        return self.params.from_coefficients(self.secret_coeffs[index], REPR_NTT)

    def __len__(self):
        return len(self.secret_coeffs)

    def to_bytes(self) -> bytearray:
        """a wire blob of kind 5: the k*l coefficients as little-endian i64 after the header.  A bytearray the caller owns
        and should wipe (blob[:] = bytes(len(blob))) when done with it; no other copy of the coefficients is made."""
        p = self.params
        head = _wire_header(p, _ffi.WIRE_SK)
        out = bytearray(len(head) + self.secret_coeffs.size * 8)
        out[:len(head)] = head.tobytes()
        np.frombuffer(out, dtype="<i8", offset=len(head))[:] = self.secret_coeffs.ravel()
        return out

    @staticmethod
    def from_bytes(params: PvwParameters, data) -> "SecretKey":
        _, _, hl, _ = _wire_check(params, data, _ffi.WIRE_SK)
        view = np.frombuffer(data, dtype="<i8", offset=hl).reshape(params.k, params.l)
        return SecretKey(params, view)


class Party:
    """Party (public_key.rs:17-22)."""

    def __init__(self, index: int, secret_key: SecretKey):
        self.index, self.secret_key = index, secret_key

    @staticmethod
    def new(index: int, params: PvwParameters, seed: bytes) -> "Party":   # :62-79
        if index >= params.n:
            raise PvwError(1, f"Party index {index} exceeds maximum {params.n - 1}")
        return Party(index, SecretKey.random(params, seed, index))


class GlobalPublicKey:
    """GlobalPublicKey (public_key.rs:43-54): the n x k matrix B lives on the device."""

    def __init__(self, crs: PvwCrs):
        self.crs = crs
        self.params = crs.params

    @staticmethod
    def new(crs: PvwCrs) -> "GlobalPublicKey":
        return GlobalPublicKey(crs)

    def add_public_key(self, index: int, key_polynomials: np.ndarray, repr: int = REPR_POWER) -> None:   # :214-250
        p = self.params
        b = _u64(key_polynomials)
        if index >= p.n:
            raise PvwError(1, f"Party index {index} exceeds maximum {p.n - 1}")
        if b.shape != (p.k, p.L, p.l):
            raise PvwError(1, f"Public key dimension {b.shape[0]} doesn't match parameter k={p.k}")
        p._call("pvw_load_pk", index, index + 1, _ptr(b), repr)

    def load_rows(self, party_lo: int, rows: np.ndarray, repr: int = REPR_POWER) -> None:
        p = self.params
        b = _u64(rows)
        p._call("pvw_load_pk", party_lo, party_lo + b.shape[0], _ptr(b), repr)

    def generate_and_add_party(self, party: Party, seed: bytes) -> None:   # :256-263
        self._keygen(party.index, party.index + 1, party.secret_key.secret_coeffs[None], None, seed)

    def generate_all_party_keys(self, parties: Sequence[Party], seed: bytes) -> None:   # :376-401
        if len(parties) > self.params.n:
            raise PvwError(1, f"Too many parties: {len(parties)} > {self.params.n}")
        # the reference generates the keys in parallel and adds them in order (:387-399); here every run of
        # consecutive party indices is ONE batched device call (the matrix-core path from 8 parties up)
        i = 0
        while i < len(parties):
            j = i + 1
            while j < len(parties) and parties[j].index == parties[j - 1].index + 1:
                j += 1
            sk = np.stack([pt.secret_key.secret_coeffs for pt in parties[i:j]])
            try:
                self._keygen(parties[i].index, parties[i].index + (j - i), sk, None, seed)
            finally:
                sk.fill(0)                                 # the stacked copy does not outlive the call, whatever happened
            i = j

    def generate_with_errors(self, party_lo: int, sk: np.ndarray, ek: np.ndarray) -> None:
        """b_i = s_i*A + e_i with explicit key errors (public_key.rs:111-147)."""
        self._keygen(party_lo, party_lo + len(sk), sk, ek, None)

    def generate_seeded(self, party_lo: int, party_hi: int, sk_seed: bytes, seed: bytes) -> None:
        """pvw_keygen_seeded: generate_all_party_keys over Party.new (public_key.rs:376-401, :62-79) with the secret keys drawn
        on the device from `sk_seed` by the kernel that transforms them -- party p's key is SecretKey.random(params, sk_seed, p) --
        and the key errors from `seed`; bit-equal to Party.new + generate_all_party_keys, without the keys on the host."""
        sk_sd, sd = _seed(sk_seed), _seed(seed)
        try:
            self.params._call("pvw_keygen_seeded", int(party_lo), int(party_hi), _ptr(sk_sd), _ptr(sd))
        finally:
            sk_sd.fill(0)

    def _keygen(self, lo, hi, sk, ek, seed):
        p = self.params
        sk = _i64(sk)
        ekp = None if ek is None else _i64(ek)
        sd = None if seed is None else _seed(seed)
        p._call("pvw_keygen", lo, hi, _ptr(sk), _ptr(ekp), _ptr(sd))

    def fill_uniform(self, seed: bytes) -> None:
        self.params._call("pvw_pk_fill_uniform", _ptr(_seed(seed)))

    def matrix(self, party_lo: int = 0, party_hi: Optional[int] = None, repr: int = REPR_POWER) -> np.ndarray:
        p = self.params
        hi = p.n if party_hi is None else party_hi
        out = np.zeros((hi - party_lo, p.k, p.L, p.l), dtype=np.uint64)
        p._call("pvw_get_pk", party_lo, hi, _ptr(out), repr)
        return out

    def get_polynomial(self, i: int, j: int, repr: int = REPR_POWER) -> Optional[np.ndarray]:   # :334-336
        p = self.params
        if not (0 <= i < p.n and 0 <= j < p.k):
            return None
        return self.matrix(i, i + 1, repr)[0, j]

    def dimensions(self) -> Tuple[int, int]:
        return self.params.n, self.params.k

    def num_public_keys(self) -> int:                                      # :344
        out = C.c_uint32()
        self.params._call("pvw_num_public_keys", C.byref(out))
        return out.value

    def is_full(self) -> bool:                                             # :349
        out = C.c_int32()
        self.params._call("pvw_is_full", C.byref(out))
        return bool(out.value)

    def to_bytes(self, party_lo: Optional[int] = None, party_hi: Optional[int] = None, repr: int = REPR_POWER) -> bytes:
        """rows [party_lo, party_hi) (default: the rows this context holds) as a wire blob of kind 3, packed on the device"""
        p = self.params
        lo = p.party_lo if party_lo is None else party_lo
        hi = p.party_hi if party_hi is None else party_hi
        if not (p.party_lo <= lo <= hi <= p.party_hi):
            raise PvwError(1, f"rows [{lo}, {hi}) are not all held by this context ([{p.party_lo}, {p.party_hi}))")
        head = _wire_header(p, _ffi.WIRE_PK, repr, lo, hi)
        blob = np.empty(len(head) + (hi - lo) * p.k * p.wire_poly_bytes() + 1, dtype=np.uint8)
        blob[:len(head)] = head
        p._call("pvw_get_pk_wire", lo, hi, _ptr(blob[len(head):]), repr)
        return blob[:-1].tobytes()

    def load_bytes(self, data) -> None:
        """add_public_key for the rows of a kind-3 blob.  Checked on the device before anything is stored: a residue >= q_i
        raises DeserializationError and leaves the key, num_public_keys and the derived copies as they were."""
        p = self.params
        repr, rg, hl, a = _wire_check(p, data, _ffi.WIRE_PK)
        body = np.ascontiguousarray(a[hl:]) if len(a) > hl else np.zeros(1, dtype=np.uint8)
        p._call("pvw_load_pk_wire", rg[0], rg[1], _ptr(body), repr)

    @staticmethod
    def from_bytes(crs: PvwCrs, data) -> "GlobalPublicKey":
        g = GlobalPublicKey(crs)
        g.load_bytes(data)
        return g


# ------------------------------------------------------------------------------------
# crypto (src/crypto)
# ------------------------------------------------------------------------------------
class PvwCiphertext:
    """PvwCiphertext (encryption.rs:15-24): c1 [k][L][l], c2 [n][L][l] in `repr`."""

    def __init__(self, c1: np.ndarray, c2: np.ndarray, params: PvwParameters, repr: int):
        self.c1, self.c2, self.params, self.repr = c1, c2, params, repr

    def __len__(self):
        return len(self.c2)

    def is_empty(self) -> bool:
        return len(self.c1) == 0 and len(self.c2) == 0

    def validate(self) -> None:                                            # :41-76
        p = self.params
        if len(self.c1) != p.k:
            raise PvwError(1, f"c1 has {len(self.c1)} components but should have k={p.k}")
        if len(self.c2) != p.n:
            raise PvwError(1, f"c2 has {len(self.c2)} components but should have n={p.n}")

    def get_party_ciphertext(self, party_index: int) -> Optional[np.ndarray]:   # :82-84
        return self.c2[party_index] if 0 <= party_index < len(self.c2) else None

    def c1_components(self):
        return self.c1

    def c2_components(self):
        return self.c2

    def to_bytes(self, party_lo: Optional[int] = None, party_hi: Optional[int] = None) -> bytes:
        """a wire blob of kind 4: the c1 rows this context holds, then c2 rows [party_lo, party_hi) (default: the parties this
        context holds), packed on the device"""
        p = self.params
        lo = p.party_lo if party_lo is None else party_lo
        hi = p.party_hi if party_hi is None else party_hi
        if not (0 <= lo <= hi <= p.n):
            raise PvwError(1, f"party range [{lo}, {hi}) outside [0, {p.n})")
        polys = _u64(np.concatenate([np.asarray(self.c1)[p.c1_lo:p.c1_hi], np.asarray(self.c2)[lo:hi]]).reshape(-1, p.L, p.l))
        head = _wire_header(p, _ffi.WIRE_CT, self.repr, p.c1_lo, p.c1_hi, lo, hi)
        blob = np.empty(len(head) + len(polys) * p.wire_poly_bytes() + 1, dtype=np.uint8)
        blob[:len(head)] = head
        p._call("pvw_wire_pack", _ptr(polys), len(polys), _ptr(blob[len(head):]))
        return blob[:-1].tobytes()

    @staticmethod
    def from_bytes(params: PvwParameters, data) -> "PvwCiphertext":
        """a kind-4 blob, unpacked and checked on the device; rows the blob does not carry are zero"""
        repr, rg, hl, a = _wire_check(params, data, _ffi.WIRE_CT)
        n1, n2 = rg[1] - rg[0], rg[3] - rg[2]
        words = np.zeros((n1 + n2, params.L, params.l), dtype=np.uint64)
        body = np.ascontiguousarray(a[hl:]) if len(a) > hl else np.zeros(1, dtype=np.uint8)
        params._call("pvw_wire_unpack", _ptr(body), n1 + n2, _ptr(words))
        c1 = np.zeros((params.k, params.L, params.l), dtype=np.uint64)
        c2 = np.zeros((params.n, params.L, params.l), dtype=np.uint64)
        c1[rg[0]:rg[1]] = words[:n1]
        c2[rg[2]:rg[3]] = words[n1:]
        return PvwCiphertext(c1, c2, params, repr)


def _randomness(params: PvwParameters, seed, r, e1, e2):
    rnd = _ffi.pvw_randomness_t()
    keep = []
    if r is not None or e1 is not None or e2 is not None:
        if r is None or e1 is None or e2 is None:
            raise PvwError(1, "explicit randomness needs r, e1 and e2")
        r, e1, e2 = _i64(r), _i64(e1), _i64(e2)
        if r.shape != (params.k, params.l) or e1.shape != (params.k, params.l) or e2.shape != (params.n, params.l):
            raise PvwError(15, "explicit randomness has the wrong shape")
        rnd.mode = _ffi.RND_EXPLICIT
        rnd.r, rnd.e1, rnd.e2 = r.ctypes.data, e1.ctypes.data, e2.ctypes.data
        keep = [r, e1, e2]
    else:
        if seed is None:
            raise PvwError(1, "encrypt needs a 32-byte seed or explicit randomness")
        rnd.mode = _ffi.RND_SEED
        sd = _seed(seed)
        C.memmove(rnd.seed, sd.ctypes.data, 32)
    return rnd, keep


def _check_state(p: "PvwParameters", randomness: "DeviceRandomness", seed, explicit=False) -> None:
    if not isinstance(randomness, DeviceRandomness):
        raise PvwError(1, "randomness must be a DeviceRandomness")
    if seed is not None or explicit:
        raise PvwError(1, "give either a seed / explicit randomness or a DeviceRandomness, not both")
    if randomness._h is None:
        raise PvwError(1, "the DeviceRandomness has been freed")
    if randomness._lib is not p._lib:
        raise PvwError(1, "the DeviceRandomness was created through another build of the library")


def encrypt(scalars: Sequence[int], global_pk: GlobalPublicKey, seed: Optional[bytes] = None, *,
            r=None, e1=None, e2=None, repr: int = REPR_NTT, randomness: Optional["DeviceRandomness"] = None) -> PvwCiphertext:
    """encrypt (encryption.rs:105-214).  `randomness`: draw from that DeviceRandomness (seed call_seed(S, c), then c + 1)
    instead of `seed` / explicit r, e1, e2."""
    p = global_pk.params
    sc = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in scalars], dtype=np.uint64)
    c1 = np.zeros((p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((p.n, p.L, p.l), dtype=np.uint64)
    if randomness is not None:
        _check_state(p, randomness, seed, r is not None or e1 is not None or e2 is not None)
        p._call("pvw_encrypt_rs", _ptr(sc), len(sc), randomness._h, _ptr(c1), _ptr(c2), repr)
    else:
        rnd, keep = _randomness(p, seed, r, e1, e2)
        p._call("pvw_encrypt", _ptr(sc), len(sc), C.byref(rnd), _ptr(c1), _ptr(c2), repr)
        del keep
    ct = PvwCiphertext(c1, c2, p, repr)
    ct.validate()                                                          # :204-211
    return ct


def encrypt_party_shares(party_shares: Sequence[int], party_index: int, global_pk: GlobalPublicKey,
                         seed: Optional[bytes] = None, **kw) -> PvwCiphertext:
    """encryption.rs:221-245."""
    n = global_pk.params.n
    if party_index >= n:
        raise PvwError(1, f"Party index {party_index} exceeds maximum {n - 1}")
    if len(party_shares) != n:
        raise PvwError(1, f"Party must provide {n} shares, got {len(party_shares)}")
    return encrypt(party_shares, global_pk, seed, **kw)


def _dealer_seed(seed: bytes, dealer: int) -> bytes:
    """Per-dealer seed for encrypt_all_party_shares: the base seed with the dealer index
    folded into its last four bytes (the reference gives every dealer a fresh thread_rng)."""
    s = bytearray(seed)
    for i in range(4):
        s[28 + i] ^= (dealer >> (8 * i)) & 0xFF
    return bytes(s)


def encrypt_all_party_shares(all_shares: Sequence[Sequence[int]], global_pk: GlobalPublicKey,
                             seed: Optional[bytes] = None, repr: int = REPR_NTT, *,
                             randomness: Optional["DeviceRandomness"] = None) -> List[PvwCiphertext]:
    """encrypt_all_party_shares (encryption.rs:253-286): one batched device call; dealers share
    passes over the public key four at a time (pvw_encrypt_multi).  Dealer d uses
    `_dealer_seed(seed, d)`, so the result equals d separate `encrypt_party_shares` calls.
    `randomness` instead of `seed`: dealer d uses call_seed(S, c + d) of that DeviceRandomness, which then holds c + n."""
    p = global_pk.params
    n = p.n
    if len(all_shares) != n:
        raise PvwError(1, f"Must provide shares for all {n} parties")
    for dealer_idx, dealer_shares in enumerate(all_shares):
        if len(dealer_shares) != n:
            raise PvwError(1, f"Dealer {dealer_idx} provided {len(dealer_shares)} shares but needs {n}")
    if randomness is not None:
        _check_state(p, randomness, seed)
        sc = np.array([[int(s) & 0xFFFFFFFFFFFFFFFF for s in row] for row in all_shares], dtype=np.uint64)
        D = sc.shape[0]
        c1 = np.zeros((D, p.k, p.L, p.l), dtype=np.uint64)
        c2 = np.zeros((D, p.n, p.L, p.l), dtype=np.uint64)
        p._call("pvw_encrypt_multi_rs", _ptr(sc), D, sc.shape[1], randomness._h, _ptr(c1), _ptr(c2), repr)
        return [PvwCiphertext(c1[d], c2[d], p, repr) for d in range(D)]
    if seed is None:
        raise PvwError(1, "encrypt_all_party_shares needs a 32-byte seed or a DeviceRandomness")
    return encrypt_many(all_shares, global_pk, [_dealer_seed(seed, d) for d in range(len(all_shares))], repr)


def encrypt_many(all_scalars: Sequence[Sequence[int]], global_pk: GlobalPublicKey, seeds: Sequence[bytes],
                 repr: int = REPR_NTT) -> List[PvwCiphertext]:
    """D independent encrypts (any D) batched through pvw_encrypt_multi."""
    p = global_pk.params
    D = len(all_scalars)
    if len(seeds) != D:
        raise PvwError(15, f"expected {D} seeds, got {len(seeds)}")
    sc = np.array([[int(s) & 0xFFFFFFFFFFFFFFFF for s in row] for row in all_scalars], dtype=np.uint64)
    if sc.ndim != 2:
        raise PvwError(1, "ragged scalar rows")
    sd = np.concatenate([_seed(s) for s in seeds]) if D else np.zeros(0, dtype=np.uint8)
    c1 = np.zeros((D, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((D, p.n, p.L, p.l), dtype=np.uint64)
    p._call("pvw_encrypt_multi", _ptr(sc), D, sc.shape[1] if D else 0, _ptr(sd), _ptr(c1), _ptr(c2), repr)
    return [PvwCiphertext(c1[d], c2[d], p, repr) for d in range(D)]


def _words(values) -> np.ndarray:
    return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in values], dtype=np.uint64)


def _seeds(seeds, D: int) -> np.ndarray:
    if len(seeds) != D:
        raise PvwError(15, f"expected {D} seeds, got {len(seeds)}")
    return np.concatenate([_seed(s) for s in seeds])


def _shamir_shares(params: PvwParameters, se: np.ndarray, pack: tuple, degree: int, plain_modulus: int, seeds, coeffs,
                   host: bool) -> np.ndarray:
    """shamir_shares (se [D], pack = ()) and shamir_shares_packed (se [D][K], pack = (K,)): pvw_shamir_shares[_packed][_host]"""
    D = len(se)
    sd = _seeds(seeds, D) if seeds is not None else None
    co = None
    if coeffs is not None:
        co = np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in coeffs], dtype=np.uint64).reshape(D, -1)
        if co.shape[1] != int(degree):
            raise PvwError(15, f"expected {int(degree)} coefficients per dealer, got {co.shape[1]}")
    out = np.zeros((D, params.n), dtype=np.uint64)
    params._call("pvw_shamir_shares" + ("_packed" if pack else "") + ("_host" if host else ""), _ptr(se), D, *pack, int(degree),
                 int(plain_modulus), _ptr(sd), _ptr(co), _ptr(out))
    return out


def _deal_party_shares(se: np.ndarray, pack: tuple, degree: int, plain_modulus: int, global_pk: GlobalPublicKey, seeds, randomness,
                       out_repr: int) -> List[PvwCiphertext]:
    """deal_party_shares (se [D], pack = ()) and deal_party_shares_packed (se [D][K], pack = (K,)): pvw_deal_shares[_packed][_rs]"""
    p = global_pk.params
    D = len(se)
    name = "deal_shares_packed" if pack else "deal_shares"
    c1 = np.zeros((D, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((D, p.n, p.L, p.l), dtype=np.uint64)
    if randomness is not None:
        _check_state(p, randomness, seeds)
        p._call(f"pvw_{name}_rs", _ptr(se), D, *pack, int(degree), int(plain_modulus), randomness._h, _ptr(c1), _ptr(c2), out_repr)
    else:
        if seeds is None:
            raise PvwError(1, f"{name.replace('deal', 'deal_party')} needs one 32-byte seed per dealer or a DeviceRandomness")
        sd = _seeds(seeds, D)
        p._call(f"pvw_{name}", _ptr(se), D, *pack, int(degree), int(plain_modulus), _ptr(sd), _ptr(c1), _ptr(c2), out_repr)
    return [PvwCiphertext(c1[d], c2[d], p, out_repr) for d in range(D)]


def shamir_shares(params: PvwParameters, secrets: Sequence[int], degree: int, plain_modulus: int,
                  seeds: Optional[Sequence[bytes]] = None, coeffs=None, host: bool = False) -> np.ndarray:
    """EXTENSION: shares[d][i] = f_d(i + 1) mod plain_modulus, f_d = secrets[d] + a_{d,1} x + ... of `degree`;
    the a_{d,j} are drawn from dealer d's 32-byte seed (stream (DOM_SHAMIR << 32) | j) or given as coeffs [D][degree].
    On the device (pvw_shamir_shares); host=True: the plain C++ restatement (pvw_shamir_shares_host, no GPU).  A sharded
    context's device call writes its own columns of the (D, n) result and leaves the others zero."""
    return _shamir_shares(params, _words(secrets), (), degree, plain_modulus, seeds, coeffs, host)


def deal_party_shares(secrets: Sequence[int], degree: int, plain_modulus: int, global_pk: GlobalPublicKey,
                      seeds: Optional[Sequence[bytes]] = None, randomness: Optional["DeviceRandomness"] = None,
                      out_repr: int = REPR_NTT) -> List[PvwCiphertext]:
    """EXTENSION: dealer d shares secrets[d] among the n parties and encrypts the shares, in one device call
    (pvw_deal_shares): what encrypt_many(shamir_shares(..., seeds), global_pk, seeds) returns, without the shares or the
    polynomial coefficients ever existing on the host.  `randomness` instead of `seeds`: dealer d uses call_seed(S, c + d)
    of that DeviceRandomness, which then holds c + D."""
    return _deal_party_shares(_words(secrets), (), degree, plain_modulus, global_pk, seeds, randomness, out_repr)


def shamir_reconstruct(indices: Sequence[int], shares, plain_modulus: int):
    """EXTENSION: the secret(s) from the shares of the parties `indices` (global indices, at least degree + 1
    of them), by Lagrange interpolation at 0 on the host (pvw_shamir_reconstruct; no GPU, no context).  shares: one value
    per index -> an int; or rows [num_secrets][len(indices)] -> a list of ints."""
    idx = _words(indices)
    single = len(shares) == 0 or np.ndim(shares[0]) == 0
    rows = [shares] if single else shares
    sh = np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in rows], dtype=np.uint64).reshape(len(rows), -1)
    if sh.shape[1] != len(idx):
        raise PvwError(15, f"expected {len(idx)} shares per secret, got {sh.shape[1]}")
    out = np.zeros(len(rows), dtype=np.uint64)
    L = _ffi.lib()
    _check(L.pvw_shamir_reconstruct(int(plain_modulus), _ptr(idx), _ptr(sh), len(idx), len(rows), _ptr(out)), L)
    return int(out[0]) if single else [int(v) for v in out]


WIDE_WORDS = 4   # PVW_WIDE_WORDS: a wide element is four little-endian uint64 words


def _wide(values) -> np.ndarray:
    """Python ints (any size: the low 256 bits) or ready-made words [..., 4] -> uint64 [N][4]"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint64 and values.ndim >= 1 and values.shape[-1] == WIDE_WORDS:
        return np.ascontiguousarray(values).reshape(-1, WIDE_WORDS)
    return np.array([[(int(v) >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(WIDE_WORDS)] for v in values],
                    dtype=np.uint64).reshape(-1, WIDE_WORDS)


def _wide_ints(words: np.ndarray) -> list:
    return [sum(int(row[w]) << (64 * w) for w in range(WIDE_WORDS)) for row in np.asarray(words).reshape(-1, WIDE_WORDS)]


def _wide_modulus(plain_modulus: int) -> np.ndarray:
    p = int(plain_modulus)
    if p < 0 or p >> 256:
        raise PvwError(1, "plain_modulus must be below 2^256")
    return _wide([p])


def shamir_wide_limbs(plain_modulus: int, limb_bits: int = 52) -> int:
    """EXTENSION: NL = ceil(bitlen(plain_modulus) / limb_bits), the ciphertexts per dealer of
    deal_party_shares_wide (pvw_shamir_wide_limbs; no GPU, no context)."""
    nl = C.c_uint32()
    L = _ffi.lib()
    _check(L.pvw_shamir_wide_limbs(_ptr(_wide_modulus(plain_modulus)), int(limb_bits), C.byref(nl)), L)
    return int(nl.value)


def shamir_shares_wide(params: PvwParameters, secrets: Sequence[int], degree: int, plain_modulus: int,
                       seeds: Optional[Sequence[bytes]] = None, coeffs=None, host: bool = False) -> np.ndarray:
    """EXTENSION: shamir_shares over an odd prime plain_modulus < 2^256.  secrets and coeffs [D][degree] are Python
    ints (any value: read mod p); the result is a uint64 array [D][n][4] of little-endian words.  On the device
    (pvw_shamir_shares_wide); host=True: the restatement on the host cores (pvw_shamir_shares_wide_host, no GPU).  A sharded
    context's device call writes its own columns and leaves the others zero."""
    se = _wide(secrets)
    D = len(se)
    sd = _seeds(seeds, D) if seeds is not None else None
    co = None
    if coeffs is not None:
        rows = [list(row) for row in coeffs]
        if any(len(row) != int(degree) for row in rows) or len(rows) != D:
            raise PvwError(15, f"expected {D} rows of {int(degree)} coefficients")
        co = _wide([v for row in rows for v in row]) if int(degree) else None     # degree 0 reads no coefficient
    out = np.zeros((D, params.n, WIDE_WORDS), dtype=np.uint64)
    params._call("pvw_shamir_shares_wide" + ("_host" if host else ""), _ptr(se), D, int(degree), _ptr(_wide_modulus(plain_modulus)),
                 _ptr(sd), _ptr(co), _ptr(out))
    return out


def deal_party_shares_wide(secrets: Sequence[int], degree: int, plain_modulus: int, global_pk: GlobalPublicKey,
                           seeds: Optional[Sequence[bytes]] = None, randomness: Optional["DeviceRandomness"] = None,
                           limb_bits: int = 52, out_repr: int = REPR_NTT) -> List[List[PvwCiphertext]]:
    """EXTENSION: dealer d shares secrets[d] over the field of plain_modulus (an odd prime below 2^256) and encrypts
    the shares limb by limb in one device call (pvw_deal_shares_wide): D lists of NL ciphertexts, ciphertext [d][w] carrying limb
    w (limb_bits bits) of dealer d's shares.  seeds: D * NL of them, vector d * NL + w's; dealer d's coefficients are drawn under
    seeds[d * NL].  `randomness` instead: vector v uses call_seed(S, c + v) and the state then holds c + D * NL."""
    p = global_pk.params
    se = _wide(secrets)
    D = len(se)
    NL = shamir_wide_limbs(plain_modulus, limb_bits)
    V = D * NL
    pm = _wide_modulus(plain_modulus)
    c1 = np.zeros((V, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((V, p.n, p.L, p.l), dtype=np.uint64)
    if randomness is not None:
        _check_state(p, randomness, seeds)
        p._call("pvw_deal_shares_wide_rs", _ptr(se), D, int(degree), _ptr(pm), int(limb_bits), randomness._h, _ptr(c1), _ptr(c2), out_repr)
    else:
        if seeds is None:
            raise PvwError(1, "deal_party_shares_wide needs one 32-byte seed per limb ciphertext or a DeviceRandomness")
        sd = _seeds(seeds, V)
        p._call("pvw_deal_shares_wide", _ptr(se), D, int(degree), _ptr(pm), int(limb_bits), _ptr(sd), _ptr(c1), _ptr(c2), out_repr)
    return [[PvwCiphertext(c1[d * NL + w], c2[d * NL + w], p, out_repr) for w in range(NL)] for d in range(D)]


def shamir_wide_to_limbs(values, limb_bits: int = 52, num_limbs: Optional[int] = None, plain_modulus: Optional[int] = None) -> np.ndarray:
    """EXTENSION: values (ints, or words [count][4]) -> uint64 limbs [num_limbs][count], limb w of value i at
    [w][i] (pvw_shamir_wide_to_limbs_host).  num_limbs, or plain_modulus to take it from shamir_wide_limbs."""
    v = _wide(values)
    nl = int(num_limbs) if num_limbs is not None else shamir_wide_limbs(plain_modulus, limb_bits)
    out = np.zeros((nl, len(v)), dtype=np.uint64)
    L = _ffi.lib()
    _check(L.pvw_shamir_wide_to_limbs_host(_ptr(v), len(v), int(limb_bits), nl, _ptr(out)), L)
    return out


def shamir_wide_from_limbs(limbs, plain_modulus: int, limb_bits: int = 52) -> list:
    """EXTENSION: limbs [num_limbs][count] (each any uint64: a limb, or a sum of limbs as decrypt_all_party_sums
    returns it) -> the ints sum_w limbs[w][i] 2^(w limb_bits) mod plain_modulus (pvw_shamir_wide_from_limbs_host)."""
    lm = np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in limbs], dtype=np.uint64)
    lm = lm.reshape(len(lm), -1)
    out = np.zeros((lm.shape[1], WIDE_WORDS), dtype=np.uint64)
    L = _ffi.lib()
    _check(L.pvw_shamir_wide_from_limbs_host(_ptr(_wide_modulus(plain_modulus)), _ptr(lm), lm.shape[1], int(limb_bits), lm.shape[0], _ptr(out)), L)
    return _wide_ints(out)


def shamir_reconstruct_wide(indices: Sequence[int], shares, plain_modulus: int):
    """EXTENSION: shamir_reconstruct over a prime below 2^256 (pvw_shamir_reconstruct_wide; host only).  shares:
    one int per index -> an int; rows [num_secrets][len(indices)] of ints, or words [num_secrets][len(indices)][4] -> a list."""
    idx = _words(indices)
    if isinstance(shares, np.ndarray) and shares.dtype == np.uint64 and shares.ndim == 3:
        single, sh = False, np.ascontiguousarray(shares)
    else:
        single = len(shares) == 0 or np.ndim(shares[0]) == 0
        rows = [shares] if single else shares
        if any(len(row) != len(idx) for row in rows):
            raise PvwError(15, f"expected {len(idx)} shares per secret")
        sh = _wide([v for row in rows for v in row]).reshape(len(rows), len(idx), WIDE_WORDS)
    if sh.shape[1] != len(idx):
        raise PvwError(15, f"expected {len(idx)} shares per secret, got {sh.shape[1]}")
    out = np.zeros((sh.shape[0], WIDE_WORDS), dtype=np.uint64)
    L = _ffi.lib()
    _check(L.pvw_shamir_reconstruct_wide(_ptr(_wide_modulus(plain_modulus)), _ptr(idx), _ptr(sh), len(idx), sh.shape[0], _ptr(out)), L)
    res = _wide_ints(out)
    return res[0] if single else res


def _wide_packed_secrets(secrets, pack: int) -> np.ndarray:
    """rows [D][pack] of ints (or words [D][pack][4]) -> uint64 [D][pack][4], dealer-major"""
    K = int(pack)
    if isinstance(secrets, np.ndarray) and secrets.dtype == np.uint64 and secrets.ndim == 3 and secrets.shape[-1] == WIDE_WORDS:
        se = np.ascontiguousarray(secrets)
        if K and se.shape[1] != K:
            raise PvwError(15, f"expected {K} secrets per dealer, got {se.shape[1]}")
        return se
    rows = [list(row) for row in secrets]
    if any(len(row) != K for row in rows):
        raise PvwError(15, f"expected {K} secrets per dealer")
    return _wide([v for row in rows for v in row]).reshape(len(rows), K, WIDE_WORDS)


def shamir_shares_packed_wide(params: PvwParameters, secrets, pack: int, degree: int, plain_modulus: int,
                              seeds: Optional[Sequence[bytes]] = None, coeffs=None, host: bool = False) -> np.ndarray:
    """EXTENSION: shamir_shares_packed over an odd prime plain_modulus < 2^256: secrets [D][pack] (ints, any value:
    read mod p) sit at the points 0, -1, .., -(pack-1) of dealer d's polynomial of degree <= degree + pack - 1, with `degree`
    random coefficients drawn as shamir_shares_wide draws them or given as coeffs [D][degree].  Returns uint64 words [D][n][4].
    On the device (pvw_shamir_shares_packed_wide); host=True: the restatement on the host cores (no GPU).  pack = 1 is
    shamir_shares_wide bit for bit."""
    se = _wide_packed_secrets(secrets, pack)
    D = len(se)
    sd = _seeds(seeds, D) if seeds is not None else None
    co = None
    if coeffs is not None:
        rows = [list(row) for row in coeffs]
        if any(len(row) != int(degree) for row in rows) or len(rows) != D:
            raise PvwError(15, f"expected {D} rows of {int(degree)} coefficients")
        co = _wide([v for row in rows for v in row]) if int(degree) else None     # degree 0 reads no coefficient
    out = np.zeros((D, params.n, WIDE_WORDS), dtype=np.uint64)
    params._call("pvw_shamir_shares_packed_wide" + ("_host" if host else ""), _ptr(se), D, int(pack), int(degree),
                 _ptr(_wide_modulus(plain_modulus)), _ptr(sd), _ptr(co), _ptr(out))
    return out


def deal_party_shares_packed_wide(secrets, pack: int, degree: int, plain_modulus: int, global_pk: GlobalPublicKey,
                                  seeds: Optional[Sequence[bytes]] = None, randomness: Optional["DeviceRandomness"] = None,
                                  limb_bits: int = 52, out_repr: int = REPR_NTT) -> List[List[PvwCiphertext]]:
    """EXTENSION: deal_party_shares_wide with `pack` secrets per dealer (secrets [D][pack]) in one polynomial: D lists
    of NL limb ciphertexts carry D * pack wide secrets (pvw_deal_shares_packed_wide).  seeds, `randomness` and the limbs as
    deal_party_shares_wide; pack = 1 gives its ciphertexts bit for bit."""
    p = global_pk.params
    se = _wide_packed_secrets(secrets, pack)
    D = len(se)
    NL = shamir_wide_limbs(plain_modulus, limb_bits)
    V = D * NL
    pm = _wide_modulus(plain_modulus)
    c1 = np.zeros((V, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((V, p.n, p.L, p.l), dtype=np.uint64)
    if randomness is not None:
        _check_state(p, randomness, seeds)
        p._call("pvw_deal_shares_packed_wide_rs", _ptr(se), D, int(pack), int(degree), _ptr(pm), int(limb_bits), randomness._h, _ptr(c1),
                _ptr(c2), out_repr)
    else:
        if seeds is None:
            raise PvwError(1, "deal_party_shares_packed_wide needs one 32-byte seed per limb ciphertext or a DeviceRandomness")
        sd = _seeds(seeds, V)
        p._call("pvw_deal_shares_packed_wide", _ptr(se), D, int(pack), int(degree), _ptr(pm), int(limb_bits), _ptr(sd), _ptr(c1), _ptr(c2),
                out_repr)
    return [[PvwCiphertext(c1[d * NL + w], c2[d * NL + w], p, out_repr) for w in range(NL)] for d in range(D)]


def shamir_reconstruct_packed_wide(indices: Sequence[int], shares, plain_modulus: int, pack: int) -> List[List[int]]:
    """EXTENSION: the `pack` secrets of each row from the shares of the parties `indices` (at least degree + pack of
    them, each below plain_modulus - pack), on the host (pvw_shamir_reconstruct_packed_wide; no GPU, no context).  shares: rows
    [num_rows][len(indices)] of ints, or words [num_rows][len(indices)][4].  Returns [num_rows][pack] ints: row r's value at -j."""
    idx = _words(indices)
    if isinstance(shares, np.ndarray) and shares.dtype == np.uint64 and shares.ndim == 3:
        sh = np.ascontiguousarray(shares)
    else:
        rows = [list(row) for row in shares]
        if any(len(row) != len(idx) for row in rows):
            raise PvwError(15, f"expected {len(idx)} shares per row")
        sh = _wide([v for row in rows for v in row]).reshape(len(rows), len(idx), WIDE_WORDS)
    if sh.shape[1] != len(idx):
        raise PvwError(15, f"expected {len(idx)} shares per row, got {sh.shape[1]}")
    K, R = int(pack), sh.shape[0]
    out = np.zeros((R, max(K, 1), WIDE_WORDS), dtype=np.uint64)
    L = _ffi.lib()
    _check(L.pvw_shamir_reconstruct_packed_wide(_ptr(_wide_modulus(plain_modulus)), K, _ptr(idx), _ptr(sh), len(idx), R, _ptr(out)), L)
    flat = _wide_ints(out)
    return [flat[r * K:(r + 1) * K] for r in range(R)]


def shamir_reconstruct_packed_wide_corrected(params: Optional[PvwParameters], plain_modulus: int, pack: int, degree: int,
                                             indices: Sequence[int], shares, erased=None, *, host: bool = False,
                                             layout: str = "secret_major"):
    """EXTENSION: the `pack` secrets of each row although up to (len(indices) - degree - pack) // 2 of its shares are
    wrong (an erased one counts half).  The wide evaluate calls take targets as party indices, so the points -j cannot be named for
    a wide p: ONE shamir_evaluate_wide_corrected call at polynomial degree degree + pack - 1 evaluates the corrected polynomials at
    the first degree + pack of `indices` -- corrected shares -- and shamir_reconstruct_packed_wide reads the secrets off them.
    Returns (secrets [num_rows][pack] as ints, nerr, col_err, err_mask) with the decode's report unchanged; a row reported
    SHAMIR_UNDECODABLE gives `pack` zeros.  pack = 1 is shamir_reconstruct_wide_corrected (rows of one secret)."""
    K, t = int(pack), int(degree)
    if K == 1:
        sec, nerr, col_err, err_mask = shamir_reconstruct_wide_corrected(params, indices, shares, t, plain_modulus, host=host,
                                                                         layout=layout, erased=erased)
        return [[s] for s in sec], nerr, col_err, err_mask
    if K < 1:
        raise PvwError(1, "pack must be at least 1")
    basis = list(indices)[:t + K]
    if len(basis) < t + K:
        raise PvwError(1, f"degree {t} with pack {K} needs at least {t + K} shares")
    values, _, nerr, col_err, err_mask = shamir_evaluate_wide_corrected(params, indices, shares, t + K - 1, plain_modulus, basis, host=host,
                                                                        layout=layout, erased=erased)
    sec = shamir_reconstruct_packed_wide(basis, values, plain_modulus, K) if len(values) else []
    sec = [[0] * K if int(nerr[r]) == SHAMIR_UNDECODABLE else row for r, row in enumerate(sec)]
    return sec, nerr, col_err, err_mask


def shamir_wide_from_limbs_device(params: PvwParameters, limbs, plain_modulus: int, limb_bits: int = 52, *,
                                  layout: str = "limb_major", num_limbs: Optional[int] = None, stream=None):
    """EXTENSION: shamir_wide_from_limbs where the limbs lie (pvw_shamir_wide_from_limbs_device).  limbs is a
    contiguous int64 device tensor of any words: layout "limb_major" is [num_limbs][count], the planes of shamir_wide_from_limbs;
    "limb_minor" is [...][num_limbs] with the limbs of one element side by side -- the [party][dealer * NL + w] values of
    decrypt_all_party_shares* read in place with num_limbs = NL, giving P * D elements in [party][dealer] order.  Returns an
    int64 device tensor [count][4] of little-endian words, made asynchronously on `stream`."""
    import torch
    if layout not in ("limb_major", "limb_minor"):
        raise ValueError(layout)
    if not hasattr(limbs, "data_ptr") or not limbs.is_contiguous() or limbs.dtype != torch.int64 or limbs.dim() < 1:
        raise PvwError(15, "limbs must be a contiguous int64 device tensor")
    if layout == "limb_major":
        nl = int(limbs.shape[0])
        count = limbs.numel() // nl if nl else 0
        strides = (max(count, 1), 1)
    else:
        nl = int(num_limbs) if num_limbs is not None else int(limbs.shape[-1])
        if nl < 1 or limbs.numel() % nl:
            raise PvwError(15, f"{limbs.numel()} words are no whole number of {nl}-limb elements")
        count = limbs.numel() // nl
        strides = (1, nl)
    out = torch.zeros((count, WIDE_WORDS), dtype=torch.int64, device=limbs.device)
    params._call("pvw_shamir_wide_from_limbs_device", _ptr(_wide_modulus(plain_modulus)), _dptr(limbs), count, strides[0], strides[1],
                 int(limb_bits), nl, _dptr(out), _stream_ptr(stream))
    return out


def shamir_wide_handover_shape(plain_modulus: int, limb_bits: int = 52, digit_bits: int = 64) -> Tuple[int, int]:
    """EXTENSION: (NL, V) of a wide handover: the limbs of a share and the signed digits of a weight,
    V = ceil((bitlen(p) + 1) / digit_bits) (pvw_shamir_wide_handover_shape; no GPU, no context)."""
    nl, nd = C.c_uint32(), C.c_uint32()
    L = _ffi.lib()
    _check(L.pvw_shamir_wide_handover_shape(_ptr(_wide_modulus(plain_modulus)), int(limb_bits), int(digit_bits), C.byref(nl), C.byref(nd)), L)
    return int(nl.value), int(nd.value)


def _handover_device(params, host: bool):
    """torch, for the device forms of the handover's public arithmetic (device pointers only: there is no host-buffer form)"""
    if host:
        return None
    if params is None:
        raise PvwError(1, "the device form needs the parameters (a context); host=True needs none")
    import torch
    return torch


def shamir_wide_signed_digits(params: Optional[PvwParameters], values, plain_modulus: int, digit_bits: int = 64, *,
                              host: bool = False) -> np.ndarray:
    """EXTENSION: the signed digits int64 [count][V] of values (ints or words [count][4], read mod p): the centred
    residue x = sum_v c_v 2^(digit_bits v), every c_v in [-2^(digit_bits-1), 2^(digit_bits-1)).  host=True:
    pvw_shamir_wide_signed_digits_host (no GPU); else the cut of the weights kernel (pvw_shamir_wide_signed_digits_device)."""
    v = _wide(values)
    V = shamir_wide_handover_shape(plain_modulus, 62, digit_bits)[1]                  # V does not depend on the limb width
    pm = _wide_modulus(plain_modulus)
    out = np.zeros((len(v), V), dtype=np.int64)
    torch = _handover_device(params, host)
    if torch is None:
        L = _ffi.lib()
        _check(L.pvw_shamir_wide_signed_digits_host(_ptr(pm), _ptr(v), len(v), int(digit_bits), _ptr(out)), L)
        return out
    dv = torch.from_numpy(v.view(np.int64)).cuda()
    do = torch.zeros((len(v), V), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    params._call("pvw_shamir_wide_signed_digits_device", _ptr(pm), _dptr(dv), len(v), int(digit_bits), _dptr(do), None)
    params.synchronize()
    return do.cpu().numpy()


def shamir_packed_wide_handover_points(plain_modulus: int, pack: int) -> List[int]:
    """EXTENSION: the points 0, -1, .., -(pack-1) of a packed wide sharing as field elements (-m is p - m), the
    `points` of shamir_wide_handover_weights for its handover."""
    p = int(plain_modulus)
    return [(p - m) % p for m in range(int(pack))]


def shamir_wide_handover_weights(params: Optional[PvwParameters], indices: Sequence[int], plain_modulus: int, valid=None, points=None,
                                 limb_bits: int = 52, digit_bits: int = 64, *, host: bool = False) -> np.ndarray:
    """EXTENSION: the int64 weight rows [T * V][D * NL] of a wide handover: row m * V + v, column d * NL + w holds
    signed digit v of lambda_{d,m} 2^(limb_bits w) mod p, lambda_{.,m} the Lagrange weights at points[m] (ints below p; None: the
    single point 0) over the points indices[d] + 1 of the valid holders; an invalid holder's columns are 0.  The rows go to
    combine_ciphertexts_many / decrypt_all_party_combinations_many over the D * NL limb ciphertexts (vector d * NL + w), and
    shamir_wide_from_digits folds the V plaintexts of a target.  host=True: pvw_shamir_wide_handover_weights_host (no GPU)."""
    idx = _words(indices)
    D = len(idx)
    v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
    if v is not None and v.shape != (D,):
        raise PvwError(15, f"valid: expected {D} flags, got {v.size}")
    pts = None if points is None else _wide([int(x) for x in points])
    if points is not None and any(int(x) < 0 or int(x) >> 256 for x in points):
        raise PvwError(1, "a target point must be a field element (the point -m is p - m)")
    T = 1 if pts is None else len(pts)
    NL, V = shamir_wide_handover_shape(plain_modulus, limb_bits, digit_bits)
    pm = _wide_modulus(plain_modulus)
    torch = _handover_device(params, host)
    if torch is None:
        out = np.zeros((T * V, D * NL), dtype=np.int64)
        L = _ffi.lib()
        _check(L.pvw_shamir_wide_handover_weights_host(_ptr(pm), _ptr(idx), _ptr(v), D, _ptr(pts), T, int(limb_bits), int(digit_bits),
                                                       _ptr(out)), L)
        return out
    do = torch.zeros((T * V, D * NL), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    params._call("pvw_shamir_wide_handover_weights_device", _ptr(pm), _ptr(idx), _ptr(v), D, _ptr(pts), T, int(limb_bits), int(digit_bits),
                 _dptr(do), None)
    params.synchronize()
    return do.cpu().numpy()


def shamir_wide_from_digits(params: Optional[PvwParameters], wide, status, plain_modulus: int, digit_bits: int = 64, *,
                            host: bool = False) -> Tuple[list, np.ndarray]:
    """EXTENSION: (values, status) from the digit plaintexts of a wide handover: wide uint64 [..][V][ww] (the
    magnitudes) and status uint32 [..][V] as decrypt_all_party_combinations_many(wide=True) reports them for R = T * V rows
    (.wide words reshaped [P][T][V][ww]); values[i] = sum_v +-|P_v| 2^(digit_bits v) mod p as ints, status[i] the OR of the V words
    without DEC_NEGATIVE.  host=True: pvw_shamir_wide_from_digits_host (no GPU)."""
    wd = np.ascontiguousarray(wide, dtype=np.uint64)
    st = np.ascontiguousarray(status, dtype=np.uint32)
    if wd.ndim < 2 or st.shape != wd.shape[:-1]:
        raise PvwError(15, "wide must be [..][V][wide_words] and status [..][V]")
    V, ww = int(wd.shape[-2]), int(wd.shape[-1])
    count = st.size // V if V else 0
    pm = _wide_modulus(plain_modulus)
    out = np.zeros((count, WIDE_WORDS), dtype=np.uint64)
    so = np.zeros(count, dtype=np.uint32)
    torch = _handover_device(params, host)
    if torch is None:
        L = _ffi.lib()
        _check(L.pvw_shamir_wide_from_digits_host(_ptr(pm), int(digit_bits), V, _ptr(wd), _ptr(st), ww, count, _ptr(out), _ptr(so)), L)
    else:
        dw = torch.from_numpy(wd.view(np.int64)).cuda()
        ds = torch.from_numpy(st.view(np.int32)).cuda()
        do = torch.zeros((count, WIDE_WORDS), dtype=torch.int64, device="cuda")
        dso = torch.zeros(count, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        params._call("pvw_shamir_wide_from_digits_device", _ptr(pm), int(digit_bits), V, _dptr(dw), _dptr(ds), ww, count, _dptr(do),
                     _dptr(dso), None)
        params.synchronize()
        out, so = do.cpu().numpy().view(np.uint64), dso.cpu().numpy().view(np.uint32)
    return _wide_ints(out), so.reshape(st.shape[:-1])


def _wide_share_matrix(indices: Sequence[int], shares, layout: str):
    """(idx, sh, S, count, strides) of the wide checked and corrected calls: the indices as words, the share matrix as uint64
    words [...][...][4], and the (secret, point) strides of `layout` in elements"""
    if layout not in ("secret_major", "party_major"):
        raise ValueError(layout)
    idx = _words(indices)
    count = len(idx)
    if isinstance(shares, np.ndarray) and shares.dtype == np.uint64 and shares.ndim == 3 and shares.shape[-1] == WIDE_WORDS:
        sh = np.ascontiguousarray(shares)
    else:
        rows = [list(row) for row in shares]
        if any(len(row) != len(rows[0]) for row in rows):
            raise PvwError(15, "the rows of shares differ in length")
        sh = _wide([v for row in rows for v in row]).reshape(len(rows), -1, WIDE_WORDS)
    S, cols = sh.shape[:2] if layout == "secret_major" else sh.shape[:2][::-1]
    if cols != count:
        raise PvwError(15, f"expected {count} shares per secret, got {cols}")
    strides = (count, 1) if layout == "secret_major" else (1, S)
    return idx, sh, S, count, strides


def shamir_reconstruct_wide_checked(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int, *,
                                    host: bool = False, layout: str = "secret_major") -> Tuple[List[int], np.ndarray, np.ndarray]:
    """EXTENSION: shamir_reconstruct_checked over an odd prime plain_modulus < 2^256.  shares: a matrix of Python
    ints (any value: the low 256 bits, read mod p) or uint64 words [...][...][4], "secret_major" [num_secrets][len(indices)] or
    "party_major" [len(indices)][num_secrets].  On the device (pvw_shamir_reconstruct_wide_checked); host=True: the plain C++
    restatement (pvw_shamir_reconstruct_wide_checked_host, no GPU; params may be None).  Returns (secrets as ints, bad, col_bad)."""
    idx, sh, S, count, strides = _wide_share_matrix(indices, shares, layout)
    out = np.zeros((S, WIDE_WORDS), dtype=np.uint64)
    bad, col_bad = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    args = (_ptr(_wide_modulus(plain_modulus)), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1], _ptr(out), _ptr(bad),
            _ptr(col_bad))
    _reconstruct_call(params, "shamir_reconstruct_wide_checked", host, args)
    return _wide_ints(out), bad, col_bad


def shamir_reconstruct_wide_corrected(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int, *,
                                      host: bool = False, layout: str = "secret_major",
                                      erased=None) -> Tuple[List[int], np.ndarray, np.ndarray, np.ndarray]:
    """EXTENSION: shamir_reconstruct_corrected over an odd prime plain_modulus < 2^256: the secrets although up to
    E = (len(indices) - degree - 1) // 2 shares of each are wrong, in whichever columns.  shares and layout as
    shamir_reconstruct_wide_checked.  On the device (pvw_shamir_reconstruct_wide_corrected); host=True: the plain C++ restatement
    (pvw_shamir_reconstruct_wide_corrected_host, Berlekamp-Welch, no GPU; params may be None).  Returns (secrets as ints, nerr,
    col_err, err_mask) as shamir_reconstruct_corrected does: an undecodable row has secret 0, nerr SHAMIR_UNDECODABLE and an empty
    mask row.
    erased: the shares KNOWN to be bad, as shamir_reconstruct_corrected takes them: a matrix of truth values in
    `layout` or packed words in the layout of err_mask (an earlier call's err_mask, or shamir_wide_erasure_mask).  Each costs one
    redundant column instead of two: row s decodes while 2 * errors + erasures <= len(indices) - degree - 1; the words at an
    erased position influence nothing and an erased column is never reported as an error.  Routes to
    pvw_shamir_reconstruct_wide_erasures*; omitted, the call is untouched."""
    idx, sh, S, count, strides = _wide_share_matrix(indices, shares, layout)
    out = np.zeros((S, WIDE_WORDS), dtype=np.uint64)
    nerr, col_err = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    err_mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    head = (_ptr(_wide_modulus(plain_modulus)), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1])
    tail = (_ptr(out), _ptr(nerr), _ptr(col_err), _ptr(err_mask))
    if erased is None:
        _reconstruct_call(params, "shamir_reconstruct_wide_corrected", host, head + tail)
    else:
        er = _erased_words(erased, S, count, layout)
        _reconstruct_call(params, "shamir_reconstruct_wide_erasures", host, head + (_ptr(er),) + tail)
    return _wide_ints(out), nerr, col_err, err_mask


def shamir_evaluate_wide_corrected(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int,
                                   targets: Sequence[int], *, host: bool = False, layout: str = "secret_major",
                                   erased=None) -> Tuple[List[List[int]], List[int], np.ndarray, np.ndarray, np.ndarray]:
    """EXTENSION: share repair over an odd prime plain_modulus < 2^256.  The decode of
    shamir_reconstruct_wide_corrected, and values[s][j] = the value of secret s's corrected polynomial at the point of party
    targets[j] (a global index below 2^64 whose point targets[j] + 1 is below plain_modulus: one of `indices` -- the share that
    party should hold -- or any other; duplicates allowed).  The row of an undecodable secret is 0.  shares and layout as
    shamir_reconstruct_wide_checked.  On the device (pvw_shamir_evaluate_wide_corrected); host=True: the plain C++ restatement
    (pvw_shamir_evaluate_wide_corrected_host, no GPU; params may be None).  Returns (values as ints [S][T], secrets as ints, nerr,
    col_err, err_mask).
    erased as shamir_reconstruct_wide_corrected (pvw_shamir_evaluate_wide_erasures*): at an erased column the value
    is the share that party should hold, which is the repair of a party that lost its state."""
    idx, sh, S, count, strides = _wide_share_matrix(indices, shares, layout)
    tg = _words(targets)
    T = len(tg)
    values = np.zeros((S, T, WIDE_WORDS), dtype=np.uint64)
    out = np.zeros((S, WIDE_WORDS), dtype=np.uint64)
    nerr, col_err = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    err_mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    head = (_ptr(_wide_modulus(plain_modulus)), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1])
    tail = (_ptr(tg), T, _ptr(values), _ptr(out), _ptr(nerr), _ptr(col_err), _ptr(err_mask))
    if erased is None:
        _reconstruct_call(params, "shamir_evaluate_wide_corrected", host, head + tail)
    else:
        er = _erased_words(erased, S, count, layout)
        _reconstruct_call(params, "shamir_evaluate_wide_erasures", host, head + (_ptr(er),) + tail)
    flat = _wide_ints(values.reshape(S * T, WIDE_WORDS)) if T else []
    return [flat[s * T:(s + 1) * T] for s in range(S)], _wide_ints(out), nerr, col_err, err_mask


def shamir_evaluate_wide_corrected_at(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int,
                                      points: Sequence[int], *, host: bool = False, layout: str = "secret_major",
                                      erased=None) -> Tuple[List[List[int]], List[int], np.ndarray, np.ndarray, np.ndarray]:
    """EXTENSION: shamir_evaluate_wide_corrected with the point of column j of the values given as the field element
    points[j] (an int in [0, plain_modulus), or words [T][4]): 0 -- the value is then the secret --, points above 2^64 and points
    that are some column's index + 1 are legal; duplicates and any order allowed.  With points[j] = targets[j] + 1 the call equals
    shamir_evaluate_wide_corrected on all five outputs.  On the device (pvw_shamir_evaluate_wide_corrected_at /
    _erasures_at); host=True: the plain C++ restatement (no GPU; params may be None).  Returns what
    shamir_evaluate_wide_corrected returns."""
    idx, sh, S, count, strides = _wide_share_matrix(indices, shares, layout)
    if not isinstance(points, np.ndarray) and any(int(x) < 0 or int(x) >> 256 for x in points):
        raise PvwError(1, "point out of range for plain_modulus")
    pts = _wide(points)
    T = len(pts)
    values = np.zeros((S, T, WIDE_WORDS), dtype=np.uint64)
    out = np.zeros((S, WIDE_WORDS), dtype=np.uint64)
    nerr, col_err = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    err_mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    head = (_ptr(_wide_modulus(plain_modulus)), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1])
    tail = (_ptr(pts), T, _ptr(values), _ptr(out), _ptr(nerr), _ptr(col_err), _ptr(err_mask))
    if erased is None:
        _reconstruct_call(params, "shamir_evaluate_wide_corrected_at", host, head + tail)
    else:
        er = _erased_words(erased, S, count, layout)
        _reconstruct_call(params, "shamir_evaluate_wide_erasures_at", host, head + (_ptr(er),) + tail)
    flat = _wide_ints(values.reshape(S * T, WIDE_WORDS)) if T else []
    return [flat[s * T:(s + 1) * T] for s in range(S)], _wide_ints(out), nerr, col_err, err_mask


def shamir_packed_wide_secrets(params: Optional[PvwParameters], plain_modulus: int, pack: int, degree: int, indices: Sequence[int],
                               shares, erased=None, *, host: bool = False, layout: str = "secret_major"):
    """EXTENSION: the `pack` secrets of each row of a packed wide sharing in ONE call, although shares
    are wrong or erased: a row is decoded at polynomial degree degree + pack - 1 and read at the points -m; it decodes while
    2 * errors + erasures <= len(indices) - degree - pack.  Every index must be below plain_modulus - pack.  shares, layout and
    erased as shamir_reconstruct_wide_corrected.  On the device (pvw_shamir_packed_wide_secrets); host=True: the plain C++
    restatement (pvw_shamir_packed_wide_secrets_host, no GPU; params may be None).  Returns (secrets [num_rows][pack] as ints,
    nerr, col_err, err_mask); a row reported SHAMIR_UNDECODABLE gives `pack` zeros.  shamir_reconstruct_packed_wide_corrected
    computes the same by the older route through t + pack corrected shares and the host."""
    idx, sh, S, count, strides = _wide_share_matrix(indices, shares, layout)
    K = int(pack)
    if K < 0 or K >> 32:
        raise PvwError(1, "pack must be at least 1")
    secrets = np.zeros((S, max(K, 1), WIDE_WORDS), dtype=np.uint64)
    nerr, col_err = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    err_mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    er = None if erased is None else _erased_words(erased, S, count, layout)
    args = (_ptr(_wide_modulus(plain_modulus)), K, int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1], _ptr(er),
            _ptr(secrets), _ptr(nerr), _ptr(col_err), _ptr(err_mask))
    _reconstruct_call(params, "shamir_packed_wide_secrets", host, args)
    flat = _wide_ints(secrets)
    return [flat[s * K:(s + 1) * K] for s in range(S)], nerr, col_err, err_mask


def _share_matrix(indices: Sequence[int], shares, layout: str):
    """(idx, sh, S, count, strides) of the checked, corrected and evaluate calls: the indices and the share matrix as uint64
    words, and the (secret, point) strides of `layout` in words"""
    if layout not in ("secret_major", "party_major"):
        raise ValueError(layout)
    idx = _words(indices)
    count = len(idx)
    sh = np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in shares], dtype=np.uint64)
    sh = sh.reshape(len(shares), -1)
    S, cols = sh.shape if layout == "secret_major" else sh.shape[::-1]
    if cols != count:
        raise PvwError(15, f"expected {count} shares per secret, got {cols}")
    strides = (count, 1) if layout == "secret_major" else (1, S)
    return idx, sh, S, count, strides


def _erased_words(erased, S: int, count: int, layout: str) -> np.ndarray:
    """the erasure mask of a call as packed words [S][ceil(count / 64)] (bit c % 64 of word c // 64 of row s: share (s, c) is
    erased): a uint64 array is taken as packed already (an err_mask, or what shamir_erasure_mask returns), anything else as a
    matrix of truth values in the call's `layout`"""
    W = (count + 63) // 64
    if isinstance(erased, np.ndarray) and erased.dtype == np.uint64:
        if erased.shape != (S, W):
            raise PvwError(15, f"expected packed erasures of shape {(S, W)}, got {erased.shape}")
        return np.ascontiguousarray(erased)
    m = np.asarray(erased).astype(bool)
    if layout == "party_major":
        m = m.T
    if m.shape != (S, count):
        raise PvwError(15, f"expected erasures for {S} secrets x {count} shares, got {m.shape}")
    bits = np.zeros((S, W * 64), dtype=np.uint8)
    bits[:, :count] = m
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint64))


def _reconstruct_call(params: Optional[PvwParameters], name: str, host: bool, args) -> None:
    """pvw_<name> on the context of params, or with host=True pvw_<name>_host (no GPU; params may be None)"""
    if host:
        L = params._lib if params is not None else _ffi.lib()
        _check(getattr(L, f"pvw_{name}_host")(*args), L)
    else:
        params._call(f"pvw_{name}", *args)


def shamir_reconstruct_checked(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int, *,
                               host: bool = False, layout: str = "secret_major") -> Tuple[List[int], np.ndarray, np.ndarray]:
    """EXTENSION: the secrets and a report on the shares they came from.  The first degree + 1 of `indices` are the
    basis: secrets[s] is the value at 0 of the polynomial through secret s's basis shares; bad[s] counts the other columns whose
    share is off that polynomial, col_bad[c] the secrets that deviate in column c.  shares: layout "secret_major" is
    [num_secrets][len(indices)] (the rows of shamir_shares), "party_major" is [len(indices)][num_secrets] (what
    decrypt_all_party_shares* returns, every dealer a secret).  On the device (pvw_shamir_reconstruct_checked); host=True: the
    plain C++ restatement (pvw_shamir_reconstruct_checked_host, no GPU; params may be None).  Returns (secrets, bad, col_bad)."""
    idx, sh, S, count, strides = _share_matrix(indices, shares, layout)
    out = np.zeros(S, dtype=np.uint64)
    bad, col_bad = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    args = (int(plain_modulus), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1], _ptr(out), _ptr(bad), _ptr(col_bad))
    _reconstruct_call(params, "shamir_reconstruct_checked", host, args)
    return [int(v) for v in out], bad, col_bad


SHAMIR_UNDECODABLE = 0xFFFFFFFF


def shamir_reconstruct_corrected(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int, *,
                                 host: bool = False, layout: str = "secret_major",
                                 erased=None) -> Tuple[List[int], np.ndarray, np.ndarray, np.ndarray]:
    """EXTENSION: the secrets although up to E = (len(indices) - degree - 1) // 2 shares of each are wrong, in
    whichever columns.  secrets[s] is the value at 0 of the one polynomial of degree <= `degree` within E columns of row s;
    nerr[s] counts the columns off it, bit c % 64 of err_mask[s][c // 64] names them and col_err[c] counts the secrets that are
    off in column c.  A row with no such polynomial: secrets[s] = 0, nerr[s] = SHAMIR_UNDECODABLE, an empty mask row.  shares and
    layout as shamir_reconstruct_checked.  On the device (pvw_shamir_reconstruct_corrected); host=True: the plain C++ restatement
    (pvw_shamir_reconstruct_corrected_host, no GPU; params may be None).  Returns (secrets, nerr, col_err, err_mask).
    erased: the shares KNOWN to be bad, a matrix of truth values in `layout` or packed words in the layout of
    err_mask (an earlier call's err_mask, or shamir_erasure_mask).  Each costs one redundant column instead of two: row s decodes
    while 2 * errors + erasures <= len(indices) - degree - 1; the word at an erased position influences nothing and an erased column
    is never reported as an error.  Routes to pvw_shamir_reconstruct_erasures*; omitted, the call is untouched."""
    idx, sh, S, count, strides = _share_matrix(indices, shares, layout)
    out = np.zeros(S, dtype=np.uint64)
    nerr, col_err = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    err_mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    head = (int(plain_modulus), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1])
    tail = (_ptr(out), _ptr(nerr), _ptr(col_err), _ptr(err_mask))
    if erased is None:
        _reconstruct_call(params, "shamir_reconstruct_corrected", host, head + tail)
    else:
        er = _erased_words(erased, S, count, layout)
        _reconstruct_call(params, "shamir_reconstruct_erasures", host, head + (_ptr(er),) + tail)
    return [int(v) for v in out], nerr, col_err, err_mask


def shamir_evaluate_corrected(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int,
                              targets: Sequence[int], *, host: bool = False, layout: str = "secret_major",
                              erased=None) -> Tuple[np.ndarray, List[int], np.ndarray, np.ndarray, np.ndarray]:
    """EXTENSION: share repair.  The decode of shamir_reconstruct_corrected, and values[s][j] = the value of secret
    s's corrected polynomial at the point of party targets[j] (a global index: one of `indices` -- the share that party should
    hold -- or any other index below plain_modulus - 1; duplicates allowed).  The row of an undecodable secret is 0.  shares and
    layout as shamir_reconstruct_checked.  On the device (pvw_shamir_evaluate_corrected); host=True: the plain C++ restatement
    (pvw_shamir_evaluate_corrected_host, no GPU; params may be None).  Returns (values, secrets, nerr, col_err, err_mask).
    erased as shamir_reconstruct_corrected (pvw_shamir_evaluate_erasures*): at an erased column the value is the
    share that party should hold, which is the repair of a party that lost its state."""
    idx, sh, S, count, strides = _share_matrix(indices, shares, layout)
    tg = _words(targets)
    values = np.zeros((S, len(tg)), dtype=np.uint64)
    out = np.zeros(S, dtype=np.uint64)
    nerr, col_err = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    err_mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    head = (int(plain_modulus), int(degree), _ptr(idx), count, _ptr(sh), S, strides[0], strides[1])
    tail = (_ptr(tg), len(tg), _ptr(values), _ptr(out), _ptr(nerr), _ptr(col_err), _ptr(err_mask))
    if erased is None:
        _reconstruct_call(params, "shamir_evaluate_corrected", host, head + tail)
    else:
        er = _erased_words(erased, S, count, layout)
        _reconstruct_call(params, "shamir_evaluate_erasures", host, head + (_ptr(er),) + tail)
    return values, [int(v) for v in out], nerr, col_err, err_mask


def shamir_erasure_mask(status=None, noise=None, *, status_bits: int = 0xFFFFFFFF, noise_bound: int = 0xFFFFFFFFFFFFFFFF,
                        layout: str = "secret_major", host: bool = False, params: Optional[PvwParameters] = None, stream=None):
    """EXTENSION: the packed erasure mask [S][ceil(count / 64)] of a decrypt report.  status (uint32) and noise
    (uint64) are matrices in `layout` ("party_major" is the [party][dealer] report of decrypt_all_party_shares_checked, every
    dealer a secret); either may be None.  Share (s, c) is erased iff status & status_bits is non-zero or noise > noise_bound
    (noise == noise_bound is not).  host=True: pvw_shamir_erasure_mask_host (no GPU); otherwise the report goes through device
    memory and pvw_shamir_erasure_mask_device on the context of `params`.  Given as device tensors (int32 status, int64 noise)
    the report is read in place, asynchronously on `stream`, and the mask comes back as a device tensor (int64 words): what
    pvw_shamir_*_erasures_device take, so decrypt-all -> mask -> decode never leaves the device."""
    if layout not in ("secret_major", "party_major"):
        raise ValueError(layout)
    if status is None and noise is None:
        raise PvwError(15, "status and noise are both None")
    if any(hasattr(a, "data_ptr") for a in (status, noise)):
        # device tensors (int32 status, int64 noise, contiguous): the mask is made where they lie and stays there, on `stream`
        import torch
        first = status if status is not None else noise
        if params is None or host or any(a is not None and (not hasattr(a, "data_ptr") or not a.is_contiguous() or a.dim() != 2
                                                             or a.shape != first.shape) for a in (status, noise)):
            raise PvwError(15, "device reports need params, host=False and contiguous matrices of one shape")
        S, count = first.shape if layout == "secret_major" else tuple(first.shape)[::-1]
        strides = (count, 1) if layout == "secret_major" else (1, S)
        d_mask = torch.zeros((S, (count + 63) // 64), dtype=torch.int64, device=first.device)
        params._call("pvw_shamir_erasure_mask_device", _dptr(status), _dptr(noise), int(status_bits), int(noise_bound), count, S,
                     strides[0], strides[1], _dptr(d_mask), _stream_ptr(stream))
        return d_mask
    st = None if status is None else np.ascontiguousarray(np.asarray(status, dtype=np.uint32))
    if noise is None:
        nz = None
    elif isinstance(noise, np.ndarray) and noise.dtype.kind in "ui":
        nz = np.ascontiguousarray(noise.astype(np.uint64, copy=False))      # a report as it came back: no walk over its elements
    else:
        nz = np.ascontiguousarray(np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in noise], dtype=np.uint64))
    shape = (st if st is not None else nz).shape
    if len(shape) != 2 or (st is not None and nz is not None and st.shape != nz.shape):
        raise PvwError(15, "status and noise must be matrices of one shape")
    S, count = shape if layout == "secret_major" else shape[::-1]
    strides = (count, 1) if layout == "secret_major" else (1, S)
    mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    if host:
        L = params._lib if params is not None else _ffi.lib()
        _check(L.pvw_shamir_erasure_mask_host(_ptr(st) if st is not None else None, _ptr(nz) if nz is not None else None,
                                              int(status_bits), int(noise_bound), count, S, strides[0], strides[1], _ptr(mask)), L)
        return mask
    if params is None:
        raise PvwError(15, "the device form needs params (or host=True)")
    import torch
    dev = torch.device("cuda", params.device) if getattr(params, "device", -1) >= 0 else torch.device("cuda")
    d_st = torch.from_numpy(st.view(np.int32)).to(dev) if st is not None else None
    d_nz = torch.from_numpy(nz.view(np.int64)).to(dev) if nz is not None else None
    d_mask = torch.zeros(mask.shape, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    params._call("pvw_shamir_erasure_mask_device", _dptr(d_st) if d_st is not None else None, _dptr(d_nz) if d_nz is not None else None,
                 int(status_bits), int(noise_bound), count, S, strides[0], strides[1], _dptr(d_mask), None)
    params.synchronize()
    return d_mask.cpu().numpy().view(np.uint64)


def shamir_wide_erasure_mask(status=None, noise=None, *, num_limbs: int, status_bits: int = 0xFFFFFFFF,
                             noise_bound: int = 0xFFFFFFFFFFFFFFFF, layout: str = "secret_major", host: bool = False,
                             params: Optional[PvwParameters] = None, stream=None):
    """EXTENSION: the packed erasure mask [S][ceil(count / 64)] of wide shares from a per-limb decrypt report.
    status (uint32) and noise (uint64) are matrices whose rows hold num_limbs consecutive entries per share: "secret_major" is
    [S][count * num_limbs], "party_major" is [count][S * num_limbs], the [party][dealer * NL + w] report of
    decrypt_all_party_shares_checked over the limb ciphertexts of deal_party_shares_wide (every dealer a secret); either may be
    None.  Share (s, c) is erased iff ONE of its limbs has status & status_bits non-zero or noise > noise_bound.  host=True:
    pvw_shamir_wide_erasure_mask_host (no GPU); otherwise pvw_shamir_wide_erasure_mask_device on the context of `params`: device
    tensors (int32 status, int64 noise) are read in place, asynchronously on `stream`, and the mask comes back as a device tensor
    (int64 words), which is what pvw_shamir_reconstruct_wide_erasures_device takes."""
    if layout not in ("secret_major", "party_major"):
        raise ValueError(layout)
    if status is None and noise is None:
        raise PvwError(15, "status and noise are both None")
    NL = int(num_limbs)

    def dims(shape):
        if len(shape) != 2 or NL <= 0 or shape[1] % NL:
            raise PvwError(15, "a report is a matrix whose rows hold num_limbs entries per share")
        S, count = (shape[0], shape[1] // NL) if layout == "secret_major" else (shape[1] // NL, shape[0])
        return S, count, ((count * NL, NL) if layout == "secret_major" else (NL, S * NL))

    if any(hasattr(a, "data_ptr") for a in (status, noise)):
        import torch
        first = status if status is not None else noise
        if params is None or host or any(a is not None and (not hasattr(a, "data_ptr") or not a.is_contiguous() or a.dim() != 2
                                                             or a.shape != first.shape) for a in (status, noise)):
            raise PvwError(15, "device reports need params, host=False and contiguous matrices of one shape")
        S, count, strides = dims(tuple(first.shape))
        d_mask = torch.zeros((S, (count + 63) // 64), dtype=torch.int64, device=first.device)
        params._call("pvw_shamir_wide_erasure_mask_device", _dptr(status), _dptr(noise), int(status_bits), int(noise_bound), count, S,
                     strides[0], strides[1], NL, 1, _dptr(d_mask), _stream_ptr(stream))
        return d_mask
    st = None if status is None else np.ascontiguousarray(np.asarray(status, dtype=np.uint32))
    if noise is None:
        nz = None
    elif isinstance(noise, np.ndarray) and noise.dtype.kind in "ui":
        nz = np.ascontiguousarray(noise.astype(np.uint64, copy=False))
    else:
        nz = np.ascontiguousarray(np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in noise], dtype=np.uint64))
    shape = (st if st is not None else nz).shape
    if st is not None and nz is not None and st.shape != nz.shape:
        raise PvwError(15, "status and noise must be matrices of one shape")
    S, count, strides = dims(shape)
    mask = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    if host:
        L = params._lib if params is not None else _ffi.lib()
        _check(L.pvw_shamir_wide_erasure_mask_host(_ptr(st) if st is not None else None, _ptr(nz) if nz is not None else None,
                                                   int(status_bits), int(noise_bound), count, S, strides[0], strides[1], NL, 1,
                                                   _ptr(mask)), L)
        return mask
    if params is None:
        raise PvwError(15, "the device form needs params (or host=True)")
    import torch
    dev = torch.device("cuda", params.device) if getattr(params, "device", -1) >= 0 else torch.device("cuda")
    d_st = torch.from_numpy(st.view(np.int32)).to(dev) if st is not None else None
    d_nz = torch.from_numpy(nz.view(np.int64)).to(dev) if nz is not None else None
    d_mask = torch.zeros(mask.shape, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    params._call("pvw_shamir_wide_erasure_mask_device", _dptr(d_st) if d_st is not None else None,
                 _dptr(d_nz) if d_nz is not None else None, int(status_bits), int(noise_bound), count, S, strides[0], strides[1], NL, 1,
                 _dptr(d_mask), None)
    params.synchronize()
    return d_mask.cpu().numpy().view(np.uint64)


def _secret_rows(secrets) -> np.ndarray:
    """secrets [D][pack] as uint64 words"""
    rows = [[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in secrets]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise PvwError(15, "expected secrets [num_dealers][pack] with pack >= 1 values in every row")
    return np.array(rows, dtype=np.uint64)


def shamir_shares_packed(params: PvwParameters, secrets, degree: int, plain_modulus: int,
                         seeds: Optional[Sequence[bytes]] = None, coeffs=None, host: bool = False) -> np.ndarray:
    """EXTENSION: packed sharing.  secrets [D][K]: dealer d's K secrets sit at the points 0, -1, ..., -(K-1) of one
    polynomial f_d = sum_j secrets[d][j] L_j + Z (a_{d,1} + ... + a_{d,degree} x^(degree-1)), Z = x (x+1) ... (x+K-1), and
    shares[d][i] = f_d(i + 1) mod plain_modulus.  The a_{d,j} are the draws of shamir_shares, or coeffs [D][degree].  K = 1 is
    shamir_shares.  On the device (pvw_shamir_shares_packed); host=True: the plain C++ restatement (no GPU).  A sharded context's
    device call writes its own columns of the (D, n) result and leaves the others zero."""
    se = _secret_rows(secrets)
    return _shamir_shares(params, se, (se.shape[1],), degree, plain_modulus, seeds, coeffs, host)


def deal_party_shares_packed(secrets, degree: int, plain_modulus: int, global_pk: GlobalPublicKey,
                             seeds: Optional[Sequence[bytes]] = None, randomness: Optional["DeviceRandomness"] = None,
                             out_repr: int = REPR_NTT) -> List[PvwCiphertext]:
    """EXTENSION: dealer d shares its K secrets secrets[d] in one polynomial and encrypts the shares, in one device
    call (pvw_deal_shares_packed): what encrypt_many(shamir_shares_packed(..., seeds), global_pk, seeds) returns, one ciphertext
    per K secrets, without the shares or the coefficients ever existing on the host.  seeds / randomness as deal_party_shares."""
    se = _secret_rows(secrets)
    return _deal_party_shares(se, (se.shape[1],), degree, plain_modulus, global_pk, seeds, randomness, out_repr)


def shamir_reconstruct_packed(indices: Sequence[int], shares, plain_modulus: int, pack: int) -> List[List[int]]:
    """EXTENSION: the `pack` secrets of every row from the shares of the parties `indices` (at least degree + pack of
    them), by Lagrange interpolation at 0, -1, ..., -(pack-1) on the host (pvw_shamir_reconstruct_packed; no GPU, no context).
    shares: rows [num_rows][len(indices)] -> [num_rows][pack] ints."""
    idx = _words(indices)
    sh = np.array([[int(v) & 0xFFFFFFFFFFFFFFFF for v in row] for row in shares], dtype=np.uint64).reshape(len(shares), -1)
    if sh.shape[1] != len(idx):
        raise PvwError(15, f"expected {len(idx)} shares per row, got {sh.shape[1]}")
    out = np.zeros((len(shares), max(int(pack), 0)), dtype=np.uint64)
    L = _ffi.lib()
    _check(L.pvw_shamir_reconstruct_packed(int(plain_modulus), int(pack), _ptr(idx), _ptr(sh), len(idx), len(shares), _ptr(out)), L)
    return [[int(v) for v in row] for row in out]


def shamir_packed_secret_indices(plain_modulus: int, pack: int) -> List[int]:
    """EXTENSION: the `targets` of shamir_evaluate_corrected that give secrets 1 .. pack-1 of a packed sharing:
    index p - 1 - j is the point -j.  (Secret 0 is the call's `out`.)"""
    return [int(plain_modulus) - 1 - j for j in range(1, int(pack))]


def shamir_reconstruct_packed_corrected(params: Optional[PvwParameters], indices: Sequence[int], shares, degree: int, plain_modulus: int,
                                        pack: int, *, host: bool = False, layout: str = "secret_major",
                                        erased=None) -> Tuple[List[List[int]], np.ndarray, np.ndarray, np.ndarray]:
    """EXTENSION: the secrets of a packed sharing although up to (len(indices) - degree - pack) // 2 shares of each
    row are wrong: one shamir_evaluate_corrected call with polynomial degree `degree + pack - 1` and the targets
    shamir_packed_secret_indices.  Returns (secrets [S][pack], nerr, col_err, err_mask): column 0 from `out`, the rest from
    `values`; an undecodable row is all 0 with nerr = SHAMIR_UNDECODABLE.  pack = 1 has no targets and is
    shamir_reconstruct_corrected.  erased is passed through."""
    if int(pack) == 1:
        out, nerr, col_err, err_mask = shamir_reconstruct_corrected(params, indices, shares, degree, plain_modulus, host=host, layout=layout,
                                                                    erased=erased)
        return [[v] for v in out], nerr, col_err, err_mask
    values, out, nerr, col_err, err_mask = shamir_evaluate_corrected(
        params, indices, shares, int(degree) + int(pack) - 1, plain_modulus, shamir_packed_secret_indices(plain_modulus, pack),
        host=host, layout=layout, erased=erased)
    secrets = [[int(out[s])] + [int(v) for v in values[s]] for s in range(len(out))]
    return secrets, nerr, col_err, err_mask


def encrypt_broadcast(scalar: int, global_pk: GlobalPublicKey, seed: Optional[bytes] = None, **kw) -> PvwCiphertext:
    """encryption.rs:292-296."""
    return encrypt([scalar] * global_pk.params.n, global_pk, seed, **kw)


def decrypt_party_shares(all_ciphertexts: Sequence[PvwCiphertext], secret_key: SecretKey, party_index: int,
                         return_noisy: bool = False):
    """decrypt_party_shares (decryption.rs:281-325): one batched device pass over all dealers."""
    if len(all_ciphertexts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p = all_ciphertexts[0].params
    if len(all_ciphertexts) != p.n:
        raise PvwError(1, f"Expected {p.n} ciphertexts, got {len(all_ciphertexts)}")
    if party_index >= p.n:
        raise PvwError(1, f"Party index {party_index} exceeds maximum {p.n - 1}")
    for d, ct in enumerate(all_ciphertexts):
        try:
            ct.validate()
        except PvwError as e:
            raise PvwError(1, f"Ciphertext {d} invalid: {e}")
    return _decrypt_batch(p, all_ciphertexts, secret_key, party_index, return_noisy)


def decrypt_many(ciphertexts: Sequence[PvwCiphertext], secret_keys: Sequence[SecretKey], party_lo: int) -> np.ndarray:
    """Parties [party_lo, party_lo + len(secret_keys)) each decrypt their share of every ciphertext given -- any number of
    them, e.g. the valid subset of examples/pvw_valid_dec.rs:201-209 -- in one call (pvw_decrypt_all): the counterpart of
    encrypt_many.  Returns uint64 [parties][ciphertexts]; row i equals decrypt_party_shares for party party_lo + i."""
    if len(ciphertexts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p = ciphertexts[0].params
    for d, ct in enumerate(ciphertexts):
        try:
            ct.validate()
        except PvwError as e:
            raise PvwError(1, f"Ciphertext {d} invalid: {e}")
    if len(secret_keys) == 0:
        return np.zeros((0, len(ciphertexts)), dtype=np.uint64)
    repr = ciphertexts[0].repr
    if any(ct.repr != repr for ct in ciphertexts):
        raise PvwError(18, "ciphertexts in different representations")
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in ciphertexts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in ciphertexts]), dtype=np.uint64)
    sk = np.ascontiguousarray(np.stack([_i64(k.secret_coeffs) for k in secret_keys]))
    out = np.zeros((len(secret_keys), len(ciphertexts)), dtype=np.uint64)
    try:
        p._call("pvw_decrypt_all", party_lo, party_lo + len(secret_keys), _ptr(sk), _ptr(c1s), _ptr(c2s), len(ciphertexts),
                repr, _ptr(out))
    finally:
        sk.fill(0)                                                         # the stacked copy of the keys (secret_key.rs:20-30)
    return out


def decrypt_all_party_shares(all_ciphertexts: Sequence[PvwCiphertext], parties: Sequence["Party"]) -> np.ndarray:
    """Every party decrypts its share from every dealer (examples/pvw.rs:138-149, tests/crypto.rs:284-287) in one call:
    results[recipient][dealer] (examples/pvw.rs:157-170) as uint64 [len(parties)][n].  An extension -- no single reference
    function; the checks are decrypt_party_shares' (decryption.rs:286-305) for each party, which must have consecutive
    indices."""
    if len(all_ciphertexts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p = all_ciphertexts[0].params
    if len(all_ciphertexts) != p.n:
        raise PvwError(1, f"Expected {p.n} ciphertexts, got {len(all_ciphertexts)}")
    if len(parties) == 0:
        return np.zeros((0, p.n), dtype=np.uint64)
    lo = parties[0].index
    for i, party in enumerate(parties):
        if party.index >= p.n:
            raise PvwError(1, f"Party index {party.index} exceeds maximum {p.n - 1}")
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    return decrypt_many(all_ciphertexts, [party.secret_key for party in parties], lo)


# ---- checked decryption ----
DEC_LOSSY = 1    # status bit: the returned word is not the plaintext P (P < 0 or P >= 2^64)
DEC_NEGATIVE = 2          # plain decode: P < 0
DEC_WIDE_TRUNCATED = 4    # plain decode: |P| does not fit the wide words asked for


class CheckedDecryption:
    """What a checked decrypt reports per share: values (the words the unchecked call returns), noise (min(max_i
    |residual_i|, 2^64 - 1), uint64), lossy (the value is not the plaintext) and valid = ~lossy & (noise <= bound).  Arrays
    of one shape: [D] for one party, [parties][D] for many.
    Plain decode (plain_modulus= / wide= of the calls below): values are exact whatever lossy says, so valid keeps
    the noise test only; negative / truncated are the two further status bits.  residues are the u64 words the call returned
    (P mod plain_modulus with a modulus); values are the same unless wide=True, which makes values an object array of Python
    integers, sign applied."""

    def __init__(self, values: np.ndarray, noise: np.ndarray, status: np.ndarray, bound: int, plain: bool = False,
                 wide: Optional[np.ndarray] = None):
        self.noise = noise
        self.status = status
        self.lossy = (status & DEC_LOSSY) != 0
        self.negative = (status & DEC_NEGATIVE) != 0
        self.truncated = (status & DEC_WIDE_TRUNCATED) != 0
        self.bound = int(bound)
        within = noise <= np.uint64(min(self.bound, (1 << 64) - 1))
        self.valid = within if plain else ~self.lossy & within
        self.residues = values                                              # the u64 words the call returned
        if wide is not None:
            flat = wide.reshape(-1, wide.shape[-1])
            ints = np.empty(flat.shape[0], dtype=object)
            for i, (row, ng) in enumerate(zip(flat, self.negative.reshape(-1))):
                v = sum(int(w) << (64 * j) for j, w in enumerate(row))
                ints[i] = -v if ng else v
            values = ints.reshape(status.shape)
        self.values = values

    def __iter__(self):                                                     # values, noise, lossy, valid = ...
        return iter((self.values, self.noise, self.lossy, self.valid))


def _plain(p: "PvwParameters", plain_modulus, wide, shape):
    """the plain options of a host-buffer call: (on, modulus, wide_words, wide array or None)"""
    m = 0 if plain_modulus is None else int(plain_modulus)
    if m and not 2 <= m < 1 << 62:
        raise PvwError(1, "plain_modulus must be in [2, 2^62)")
    ww = (p.q_total().bit_length() + 63) // 64 if wide else 0
    return bool(m or ww), m, ww, (np.zeros(tuple(shape) + (ww,), dtype=np.uint64) if ww else None)


def _bound(p: "PvwParameters", bound) -> int:
    b = p.noise_bound() if bound is None else int(bound)
    if b < 0:
        raise PvwError(1, "the noise bound must be non-negative")
    return b


def decrypt_party_shares_checked(all_ciphertexts: Sequence[PvwCiphertext], secret_key: SecretKey, party_index: int,
                                 bound: Optional[int] = None, *, plain_modulus: Optional[int] = None,
                                 wide: bool = False) -> CheckedDecryption:
    """decrypt_party_shares (decryption.rs:281-325) with each share's report (pvw_decrypt_batch_checked): the same
    checks and values, plus noise / lossy / valid against `bound` (default: noise_bound()).  plain_modulus / wide: the
    plain decode (pvw_decrypt_batch_plain) -- values mod plain_modulus, or as exact Python integers."""
    if len(all_ciphertexts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p = all_ciphertexts[0].params
    if len(all_ciphertexts) != p.n:
        raise PvwError(1, f"Expected {p.n} ciphertexts, got {len(all_ciphertexts)}")
    if party_index >= p.n:
        raise PvwError(1, f"Party index {party_index} exceeds maximum {p.n - 1}")
    for d, ct in enumerate(all_ciphertexts):
        try:
            ct.validate()
        except PvwError as e:
            raise PvwError(1, f"Ciphertext {d} invalid: {e}")
    return _decrypt_batch_checked(p, all_ciphertexts, secret_key, party_index, _bound(p, bound), plain_modulus, wide)


def decrypt_party_value_checked(ciphertext: PvwCiphertext, secret_key: SecretKey, party_index: int,
                                bound: Optional[int] = None) -> Tuple[int, int, bool, bool]:
    """decrypt_party_value (decryption.rs:249-278) with its report: (value, noise, lossy, valid)."""
    r = _decrypt_batch_checked(ciphertext.params, [ciphertext], secret_key, party_index, _bound(ciphertext.params, bound))
    return int(r.values[0]), int(r.noise[0]), bool(r.lossy[0]), bool(r.valid[0])


def _decrypt_batch_checked(p, cts, secret_key, party_index, bound, plain_modulus=None, wide=False) -> CheckedDecryption:
    repr = cts[0].repr
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2col = np.ascontiguousarray(np.stack([ct.c2[party_index] for ct in cts]), dtype=np.uint64)
    sk = _i64(secret_key.secret_coeffs)
    out = np.zeros(len(cts), dtype=np.uint64)
    noise = np.zeros(len(cts), dtype=np.uint64)
    status = np.zeros(len(cts), dtype=np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape)
    if on:
        p._call("pvw_decrypt_batch_plain", _ptr(sk), _ptr(c1s), _ptr(c2col), len(cts), repr, _ptr(out), _ptr(noise),
                _ptr(status), m, ww, _ptr(wd))
        return CheckedDecryption(out, noise, status, bound, True, wd)
    p._call("pvw_decrypt_batch_checked", _ptr(sk), _ptr(c1s), _ptr(c2col), len(cts), repr, _ptr(out), _ptr(noise),
            _ptr(status))
    return CheckedDecryption(out, noise, status, bound)


def decrypt_many_checked(ciphertexts: Sequence[PvwCiphertext], secret_keys: Sequence[SecretKey], party_lo: int,
                         bound: Optional[int] = None, *, plain_modulus: Optional[int] = None,
                         wide: bool = False) -> CheckedDecryption:
    """decrypt_many with each share's report (pvw_decrypt_all_checked): values, noise, lossy, valid as [parties][D].
    plain_modulus / wide: the plain decode (pvw_decrypt_all_plain)."""
    if len(ciphertexts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p = ciphertexts[0].params
    for d, ct in enumerate(ciphertexts):
        try:
            ct.validate()
        except PvwError as e:
            raise PvwError(1, f"Ciphertext {d} invalid: {e}")
    b = _bound(p, bound)
    shape = (len(secret_keys), len(ciphertexts))
    if len(secret_keys) == 0:
        return CheckedDecryption(np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), np.zeros(shape, np.uint32), b)
    repr = ciphertexts[0].repr
    if any(ct.repr != repr for ct in ciphertexts):
        raise PvwError(18, "ciphertexts in different representations")
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in ciphertexts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in ciphertexts]), dtype=np.uint64)
    sk = np.ascontiguousarray(np.stack([_i64(k.secret_coeffs) for k in secret_keys]))
    out = np.zeros(shape, dtype=np.uint64)
    noise = np.zeros(shape, dtype=np.uint64)
    status = np.zeros(shape, dtype=np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, shape)
    try:
        if on:
            p._call("pvw_decrypt_all_plain", party_lo, party_lo + len(secret_keys), _ptr(sk), _ptr(c1s), _ptr(c2s),
                    len(ciphertexts), repr, _ptr(out), _ptr(noise), _ptr(status), m, ww, _ptr(wd))
        else:
            p._call("pvw_decrypt_all_checked", party_lo, party_lo + len(secret_keys), _ptr(sk), _ptr(c1s), _ptr(c2s),
                    len(ciphertexts), repr, _ptr(out), _ptr(noise), _ptr(status))
    finally:
        sk.fill(0)                                                         # the stacked copy of the keys (secret_key.rs:20-30)
    return CheckedDecryption(out, noise, status, b, on, wd)


def decrypt_all_party_shares_checked(all_ciphertexts: Sequence[PvwCiphertext], parties: Sequence["Party"],
                                     bound: Optional[int] = None) -> CheckedDecryption:
    """decrypt_all_party_shares with each share's report: its checks, then decrypt_many_checked."""
    if len(all_ciphertexts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p = all_ciphertexts[0].params
    if len(all_ciphertexts) != p.n:
        raise PvwError(1, f"Expected {p.n} ciphertexts, got {len(all_ciphertexts)}")
    lo = parties[0].index if len(parties) else 0
    for i, party in enumerate(parties):
        if party.index >= p.n:
            raise PvwError(1, f"Party index {party.index} exceeds maximum {p.n - 1}")
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    return decrypt_many_checked(all_ciphertexts, [party.secret_key for party in parties], lo, bound)


# ---- sums of dealers' ciphertexts ----
def _sum_inputs(cts: Sequence[PvwCiphertext], valid):
    """the checks every sum shares: (params, repr, valid as uint8 [D] or None)"""
    if len(cts) == 0:
        raise PvwError(1, "No ciphertexts provided")
    p, repr = cts[0].params, cts[0].repr
    shape1, shape2 = (p.k, p.L, p.l), (p.n, p.L, p.l)
    for d, ct in enumerate(cts):
        if ct.params is not p and (ct.params.n, ct.params.k, ct.params.l, list(ct.params.moduli())) != (p.n, p.k, p.l, list(p.moduli())):
            raise PvwError(15, f"Ciphertext {d} belongs to other parameters")
        if np.shape(ct.c1) != shape1 or np.shape(ct.c2) != shape2:
            raise PvwError(15, f"Ciphertext {d}: expected c1 {shape1} and c2 {shape2}, got {np.shape(ct.c1)} and {np.shape(ct.c2)}")
        if ct.repr != repr:
            raise PvwError(15, f"Ciphertext {d} is in representation {ct.repr}, ciphertext 0 in {repr}")
    v = None
    if valid is not None:
        v = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        if v.shape != (len(cts),):
            raise PvwError(15, f"valid: expected {len(cts)} flags, got {v.size}")
    if v is not None and not v.any():
        raise PvwError(17, f"No valid dealer among the {len(cts)} ciphertexts: expected at least 1, got 0")
    return p, repr, v


def aggregate_ciphertexts(cts: Sequence[PvwCiphertext], valid=None, *, host: bool = False) -> PvwCiphertext:
    """The sum of the valid dealers' ciphertexts (pvw_ct_sum): a ciphertext of the sum of their shares under the same keys,
    in the same representation; no key is needed.  valid: one flag per ciphertext (None = all).  host=True computes it on
    the host cores (pvw_ct_sum_host, no GPU).  Its noise is the sum of the dealers' noises (PvwParameters.sum_capacity)."""
    p, repr, v = _sum_inputs(cts, valid)
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
    c1 = np.zeros((p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((p.n, p.L, p.l), dtype=np.uint64)
    p._call("pvw_ct_sum_host" if host else "pvw_ct_sum", _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), 0, p.n, _ptr(c1), _ptr(c2), None)
    return PvwCiphertext(c1, c2, p, repr)


def _sum_bound(p, bound, count: int) -> int:
    return _bound(p, count * p.noise_bound() if bound is None else bound)


def decrypt_party_sum(cts: Sequence[PvwCiphertext], secret_key: SecretKey, party_index: int, valid=None,
                      bound: Optional[int] = None, *, plain_modulus: Optional[int] = None, wide: bool = False) -> CheckedDecryption:
    """Party party_index's aggregate share -- the sum of its shares from the valid dealers (examples/pvw_valid_dec.rs:201-209)
    -- from ONE decrypt of the summed ciphertext (pvw_decrypt_sum_checked).  Arrays of shape [1]; bound defaults to
    count * noise_bound().  plain_modulus / wide: the plain decode (pvw_decrypt_sum_plain) -- the sum of the
    shares mod plain_modulus, or as an exact Python integer, where the u64 word of a field-sized sum is 0."""
    p, repr, v = _sum_inputs(cts, valid)
    if not 0 <= party_index < p.n:
        raise PvwError(1, f"Party index {party_index} exceeds maximum {p.n - 1}")
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2col = np.ascontiguousarray(np.stack([ct.c2[party_index] for ct in cts]), dtype=np.uint64)
    sk = _i64(secret_key.secret_coeffs)
    out, noise, status, count = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint32), C.c_uint32()
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape)
    if on:
        p._call("pvw_decrypt_sum_plain", _ptr(sk), _ptr(c1s), _ptr(c2col), len(cts), _ptr(v), repr, _ptr(out), _ptr(noise),
                _ptr(status), C.byref(count), m, ww, _ptr(wd))
    else:
        p._call("pvw_decrypt_sum_checked", _ptr(sk), _ptr(c1s), _ptr(c2col), len(cts), _ptr(v), repr, _ptr(out), _ptr(noise),
                _ptr(status), C.byref(count))
    return CheckedDecryption(out, noise, status, _sum_bound(p, bound, count.value), on, wd)


def decrypt_all_party_sums(cts: Sequence[PvwCiphertext], parties: Sequence["Party"], valid=None,
                           bound: Optional[int] = None, *, plain_modulus: Optional[int] = None,
                           wide: bool = False) -> CheckedDecryption:
    """Every party's aggregate share in one call (pvw_decrypt_all_sum_checked): arrays of shape [len(parties)].  The parties
    must have consecutive indices; bound defaults to count * noise_bound().  plain_modulus / wide: the plain decode
    (pvw_decrypt_all_sum_plain)."""
    p, repr, v = _sum_inputs(cts, valid)
    count = int(v.sum()) if v is not None else len(cts)
    b = _sum_bound(p, bound, count)
    if len(parties) == 0:
        return CheckedDecryption(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), b)
    lo = parties[0].index
    for i, party in enumerate(parties):
        if party.index >= p.n:
            raise PvwError(1, f"Party index {party.index} exceeds maximum {p.n - 1}")
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
    sk = np.ascontiguousarray(np.stack([_i64(party.secret_key.secret_coeffs) for party in parties]))
    out, noise, status = np.zeros(len(parties), np.uint64), np.zeros(len(parties), np.uint64), np.zeros(len(parties), np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape)
    try:
        if on:
            p._call("pvw_decrypt_all_sum_plain", lo, lo + len(parties), _ptr(sk), _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), repr,
                    _ptr(out), _ptr(noise), _ptr(status), None, m, ww, _ptr(wd))
        else:
            p._call("pvw_decrypt_all_sum_checked", lo, lo + len(parties), _ptr(sk), _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), repr,
                    _ptr(out), _ptr(noise), _ptr(status), None)
    finally:
        sk.fill(0)                                                         # the stacked copy of the keys (secret_key.rs:20-30)
    return CheckedDecryption(out, noise, status, b, on, wd)


# ---- weighted sums of dealers' ciphertexts ----
def _weights(weights, D: int, v) -> np.ndarray:
    """the checks the combination calls add to _sum_inputs: one int64 per ciphertext, at least one participating dealer"""
    w = [int(x) for x in weights]
    if len(w) != D:
        raise PvwError(15, f"weights: expected {D} weights, got {len(w)}")
    for d, x in enumerate(w):
        if not -(1 << 63) <= x < 1 << 63:
            raise PvwError(1, f"weights[{d}] = {x} is outside the int64 range")
    w = np.array(w, dtype=np.int64)
    if not ((w != 0) & (True if v is None else v != 0)).any():
        raise PvwError(17, f"No participating dealer (valid, weight not 0) among the {D} ciphertexts: expected at least 1, got 0")
    return w


def _abs_weight_sum(w: np.ndarray, v) -> int:
    return sum(abs(int(x)) for d, x in enumerate(w) if v is None or v[d])


def _lincomb_report(p, out, noise, status, w, v, bound, on, wd) -> "CheckedDecryption":
    """The report of a combination.  bound defaults to (sum of |w_d| over the participating dealers) * noise_bound(); the
    noise word saturates at 2^64 - 1, so when the bound does not fit 64 bits `valid` takes PvwParameters.lincomb_fits(weights,
    valid) in place of the noise test (the same for every entry)."""
    b = _bound(p, _abs_weight_sum(w, v) * p.noise_bound() if bound is None else bound)
    r = CheckedDecryption(out, noise, status, b, on, wd)
    if b >= 1 << 64:
        fits = np.full(status.shape, p.lincomb_fits(w, v), dtype=bool)
        r.valid = fits if on else ~r.lossy & fits
    return r


def combine_ciphertexts(cts: Sequence[PvwCiphertext], weights, valid=None, *, host: bool = False) -> PvwCiphertext:
    """sum_d weights[d] * cts[d] over the participating dealers (valid and weight not 0; pvw_ct_lincomb): a ciphertext of
    sum_d w_d m_d under the same keys, in the same representation; no key is needed.  weights: one Python integer in the int64
    range per ciphertext, read as the integer it is.  host=True computes it on the host cores (pvw_ct_lincomb_host, no GPU).
    Its noise is sum_d |w_d| noise_d (PvwParameters.lincomb_fits)."""
    p, repr, v = _sum_inputs(cts, valid)
    w = _weights(weights, len(cts), v)
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
    c1 = np.zeros((p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((p.n, p.L, p.l), dtype=np.uint64)
    p._call("pvw_ct_lincomb_host" if host else "pvw_ct_lincomb", _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), _ptr(w), 0, p.n, _ptr(c1),
            _ptr(c2), None)
    return PvwCiphertext(c1, c2, p, repr)


def decrypt_party_combination(cts: Sequence[PvwCiphertext], weights, secret_key: SecretKey, party_index: int, valid=None,
                              plain_modulus: Optional[int] = None, wide: bool = False, *, bound: Optional[int] = None) -> CheckedDecryption:
    """Party party_index's share of the combination sum_d w_d m_d from ONE decrypt (pvw_decrypt_lincomb_plain): with the
    Lagrange weights of the valid old holders and plain_modulus = p, the party's new share after a handover.  Arrays of shape
    [1].  `valid` of the report: see _lincomb_report -- with field-sized weights the noise word is saturated and
    lincomb_fits stands in for the noise test."""
    p, repr, v = _sum_inputs(cts, valid)
    w = _weights(weights, len(cts), v)
    if not 0 <= party_index < p.n:
        raise PvwError(1, f"Party index {party_index} exceeds maximum {p.n - 1}")
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2col = np.ascontiguousarray(np.stack([ct.c2[party_index] for ct in cts]), dtype=np.uint64)
    sk = _i64(secret_key.secret_coeffs)
    out, noise, status = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape)
    p._call("pvw_decrypt_lincomb_plain", _ptr(sk), _ptr(c1s), _ptr(c2col), len(cts), _ptr(v), _ptr(w), repr, _ptr(out), _ptr(noise),
            _ptr(status), None, m, ww, _ptr(wd))
    return _lincomb_report(p, out, noise, status, w, v, bound, on, wd)


def decrypt_all_party_combinations(cts: Sequence[PvwCiphertext], weights, parties: Sequence["Party"], valid=None,
                                   plain_modulus: Optional[int] = None, wide: bool = False, *,
                                   bound: Optional[int] = None) -> CheckedDecryption:
    """Every party's share of the combination in one call (pvw_decrypt_all_lincomb_plain): arrays of shape [len(parties)].  The
    parties must have consecutive indices.  `valid` of the report as decrypt_party_combination."""
    p, repr, v = _sum_inputs(cts, valid)
    w = _weights(weights, len(cts), v)
    if len(parties) == 0:
        return _lincomb_report(p, np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), w, v, bound, False, None)
    lo = parties[0].index
    for i, party in enumerate(parties):
        if party.index >= p.n:
            raise PvwError(1, f"Party index {party.index} exceeds maximum {p.n - 1}")
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
    sk = np.ascontiguousarray(np.stack([_i64(party.secret_key.secret_coeffs) for party in parties]))
    out, noise, status = np.zeros(len(parties), np.uint64), np.zeros(len(parties), np.uint64), np.zeros(len(parties), np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape)
    try:
        p._call("pvw_decrypt_all_lincomb_plain", lo, lo + len(parties), _ptr(sk), _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), _ptr(w),
                repr, _ptr(out), _ptr(noise), _ptr(status), None, m, ww, _ptr(wd))
    finally:
        sk.fill(0)                                                         # the stacked copy of the keys (secret_key.rs:20-30)
    return _lincomb_report(p, out, noise, status, w, v, bound, on, wd)


def shamir_lagrange_weights(indices: Sequence[int], plain_modulus: int) -> List[int]:
    """The Lagrange weights at 0 of the points indices[i] + 1 mod plain_modulus, centred in (-p/2, p/2]
    (pvw_shamir_lagrange_weights; host only, the argument rules of shamir_reconstruct)."""
    idx = _words(indices)
    out = np.zeros(len(idx), dtype=np.int64)
    _check(_ffi.lib().pvw_shamir_lagrange_weights(int(plain_modulus), _ptr(idx), len(idx), _ptr(out)))
    return [int(x) for x in out]


# ---- many combinations of the same dealers' ciphertexts ----
def shamir_lagrange_weights_at(indices: Sequence[int], targets: Sequence[int], plain_modulus: int) -> List[List[int]]:
    """Row j: the Lagrange weights AT the point (targets[j] + 1) mod plain_modulus of the points indices[i] + 1, centred in
    (-p/2, p/2] (pvw_shamir_lagrange_weights_at; host only).  The target p - 1 is the point 0 (shamir_lagrange_weights), p - 1 - m
    the point -m; a target that is one of the indices gives that unit vector."""
    idx, tg = _words(indices), _words(targets)
    out = np.zeros((len(tg), len(idx)), dtype=np.int64)
    _check(_ffi.lib().pvw_shamir_lagrange_weights_at(int(plain_modulus), _ptr(idx), len(idx), _ptr(tg), len(tg), _ptr(out)))
    return [[int(x) for x in row] for row in out]


def shamir_packed_handover_weights(indices: Sequence[int], plain_modulus: int, pack: int) -> List[List[int]]:
    """The weight rows of a packed sharing's handover: row m = the Lagrange weights at the point -m (secret m of
    shamir_shares_packed) of the old holders `indices`, m < pack."""
    p = int(plain_modulus)
    return shamir_lagrange_weights_at(indices, [p - 1 - m for m in range(int(pack))], p)


def _weight_rows(weight_rows, D: int, v) -> np.ndarray:
    """int64 [R][D]; at least one row, and at least one dealer that takes part in some row"""
    rows = [[int(x) for x in row] for row in weight_rows]
    if len(rows) == 0:
        raise PvwError(1, "num_combos must be at least 1")
    for r, row in enumerate(rows):
        if len(row) != D:
            raise PvwError(15, f"weight_rows[{r}]: expected {D} weights, got {len(row)}")
        for d, x in enumerate(row):
            if not -(1 << 63) <= x < 1 << 63:
                raise PvwError(1, f"weight_rows[{r}][{d}] = {x} is outside the int64 range")
    w = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(len(rows), D))
    if not ((w != 0).any(axis=0) & (True if v is None else v != 0)).any():
        raise PvwError(17, f"No participating dealer (valid, weight not 0) among the {D} ciphertexts: expected at least 1, got 0")
    return w


def combine_ciphertexts_many(cts: Sequence[PvwCiphertext], weight_rows, valid=None, *, host: bool = False) -> List[PvwCiphertext]:
    """One combination per row of weight_rows [R][D] over the same ciphertexts (pvw_ct_lincomb_many): element r is
    combine_ciphertexts(cts, weight_rows[r], valid) bit for bit -- all zeros for a row nobody takes part in -- with every
    ciphertext read once per tile of rows and uploaded once.  host=True: pvw_ct_lincomb_many_host, no GPU."""
    p, repr, v = _sum_inputs(cts, valid)
    w = _weight_rows(weight_rows, len(cts), v)
    R = w.shape[0]
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
    c1 = np.zeros((R, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((R, p.n, p.L, p.l), dtype=np.uint64)
    p._call("pvw_ct_lincomb_many_host" if host else "pvw_ct_lincomb_many", _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), _ptr(w), R, 0, p.n,
            _ptr(c1), _ptr(c2), None)
    return [PvwCiphertext(c1[r], c2[r], p, repr) for r in range(R)]


def decrypt_all_party_combinations_many(cts: Sequence[PvwCiphertext], weight_rows, parties: Sequence["Party"], valid=None,
                                        plain_modulus: Optional[int] = None, wide: bool = False, *,
                                        bound: Optional[int] = None) -> CheckedDecryption:
    """Every party's share of every combination in one call (pvw_decrypt_all_lincomb_many_plain): arrays of shape
    [len(parties)][R], column r what decrypt_all_party_combinations gives with weight_rows[r].  With
    shamir_packed_handover_weights and plain_modulus = p: values[j][m] is new party j's share of the packed sharing's secret m.
    `valid` of the report follows the rule of decrypt_party_combination row by row; .bound is the largest row's."""
    p, repr, v = _sum_inputs(cts, valid)
    w = _weight_rows(weight_rows, len(cts), v)
    R, NP = w.shape[0], len(parties)
    lo = parties[0].index if NP else 0
    for i, party in enumerate(parties):
        if party.index >= p.n:
            raise PvwError(1, f"Party index {party.index} exceeds maximum {p.n - 1}")
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    out, noise, status = np.zeros((NP, R), np.uint64), np.zeros((NP, R), np.uint64), np.zeros((NP, R), np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape) if NP else (False, 0, 0, None)
    if NP:
        c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
        c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
        sk = np.ascontiguousarray(np.stack([_i64(party.secret_key.secret_coeffs) for party in parties]))
        try:
            p._call("pvw_decrypt_all_lincomb_many_plain", lo, lo + NP, _ptr(sk), _ptr(c1s), _ptr(c2s), len(cts), _ptr(v), _ptr(w), R,
                    repr, _ptr(out), _ptr(noise), _ptr(status), None, m, ww, _ptr(wd))
        finally:
            sk.fill(0)                                                     # the stacked copy of the keys (secret_key.rs:20-30)
    rows = [_lincomb_report(p, out[:, r], noise[:, r], status[:, r], w[r], v, bound, on, None) for r in range(R)]
    rep = CheckedDecryption(out, noise, status, max(x.bound for x in rows), on, wd)
    rep.valid = np.stack([x.valid for x in rows], axis=1) if NP else np.zeros((0, R), dtype=bool)
    return rep


def decrypt_all_party_handover_wide(cts: Sequence[Sequence[PvwCiphertext]], parties: Sequence["Party"], indices: Sequence[int],
                                    plain_modulus: int, valid=None, points=None, limb_bits: int = 52,
                                    digit_bits: int = 64) -> Tuple[List[List[int]], np.ndarray]:
    """EXTENSION: the handover of a wide sharing in one call (pvw_decrypt_all_handover_wide).  cts [D][NL] are the
    old holders' re-dealt limb ciphertexts (deal_party_shares_wide's lists, holder d at party index indices[d]); `valid` masks
    holders out; points are ints below p (None: the point 0; shamir_packed_wide_handover_points for a packed old sharing).
    Returns (values [P][T] as ints, status uint32 [P][T]): values[j][m] = sum_d lambda_{d,m} f_d(j + 1) mod p, new party j's share
    of the secret at points[m], from V decrypts a party and target; status is the OR of the digit decodes' status words without
    DEC_NEGATIVE.  PvwParameters.wide_handover_fits says beforehand whether the decode is proven exact."""
    rows = [list(r) for r in cts]
    D, NL = len(rows), shamir_wide_limbs(plain_modulus, limb_bits)
    if D == 0 or any(len(r) != NL for r in rows):
        raise PvwError(15, f"expected rows of {NL} limb ciphertexts")
    flat = [ct for r in rows for ct in r]
    p, repr, _ = _sum_inputs(flat, None)
    idx = _words(indices)
    if len(idx) != D:
        raise PvwError(15, f"indices: expected {D} holders, got {len(idx)}")
    v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
    if v is not None and v.shape != (D,):
        raise PvwError(15, f"valid: expected {D} flags, got {v.size}")
    pts = None if points is None else _wide([int(x) for x in points])
    T, NP = (1 if pts is None else len(pts)), len(parties)
    lo = parties[0].index if NP else 0
    for i, party in enumerate(parties):
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    out, status, count = np.zeros((NP, T, WIDE_WORDS), np.uint64), np.zeros((NP, T), np.uint32), C.c_uint32()
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in flat]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in flat]), dtype=np.uint64)
    sk = np.ascontiguousarray(np.stack([_i64(party.secret_key.secret_coeffs) for party in parties])) if NP else np.zeros(1, np.int64)
    try:
        p._call("pvw_decrypt_all_handover_wide", lo, lo + NP, _ptr(sk), _ptr(c1s), _ptr(c2s), D, _ptr(_wide_modulus(plain_modulus)),
                int(limb_bits), int(digit_bits), _ptr(idx), _ptr(v), _ptr(pts), T, repr, _ptr(out), _ptr(status), C.byref(count))
    finally:
        sk.fill(0)                                                         # the stacked copy of the keys (secret_key.rs:20-30)
    vals = _wide_ints(out)
    return [vals[j * T:(j + 1) * T] for j in range(NP)], status


# ---- the one-word handover from a mask that may be made on the device ----
def _holder_mask(valid, D: int):
    """(host uint8 [D] or None, device tensor or None): a device tensor (uint8 / bool, contiguous, [D]) is used in place"""
    if valid is None:
        return None, None
    if hasattr(valid, "data_ptr"):
        if valid.dim() != 1 or valid.shape[0] != D or valid.element_size() != 1 or not valid.is_contiguous():
            raise PvwError(15, f"valid: expected a contiguous device tensor of {D} bytes")
        return None, valid
    v = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
    if v.shape != (D,):
        raise PvwError(15, f"valid: expected {D} flags, got {v.size}")
    return v, None


def shamir_handover_weights(params: Optional[PvwParameters], indices: Sequence[int], plain_modulus: int, valid=None, targets=None, *,
                            host: bool = False, stream=None):
    """EXTENSION: the int64 weight rows [T][D] of a one-word handover: row j = the Lagrange weights AT the point
    (targets[j] + 1) mod p (None: the single point 0; the target rule of shamir_lagrange_weights_at) over the points indices[d] + 1
    of the holders with valid[d] != 0, centred; a masked holder's column is 0.  Returns (weights, count of valid holders).
    host=True: pvw_shamir_handover_weights_host (no GPU).  Otherwise pvw_shamir_handover_weights_device: `valid` as a device tensor
    (uint8 [D]) is read in place when the kernels run, asynchronously on `stream`, and (weights, count) come back as device tensors."""
    idx = _words(indices)
    D = len(idx)
    v, dv = _holder_mask(valid, D)
    tg = None if targets is None else _words(targets)
    T = 1 if tg is None else len(tg)
    count = C.c_uint32()
    if host:
        if dv is not None:
            raise PvwError(15, "host=True takes a host mask")
        out = np.zeros((T, D), dtype=np.int64)
        L = _ffi.lib()
        _check(L.pvw_shamir_handover_weights_host(int(plain_modulus), _ptr(idx), _ptr(v), D, _ptr(tg), T, _ptr(out), C.byref(count)), L)
        return out, int(count.value)
    if params is None:
        raise PvwError(1, "the device form needs the parameters (a context); host=True needs none")
    import torch
    in_place = dv is not None
    if v is not None:
        dv = torch.from_numpy(v).cuda()
    do = torch.zeros((T, D), dtype=torch.int64, device="cuda")
    dc = torch.zeros(1, dtype=torch.int32, device="cuda")
    if not in_place:
        torch.cuda.synchronize()
    params._call("pvw_shamir_handover_weights_device", int(plain_modulus), _ptr(idx), _dptr(dv), D, _ptr(tg), T, _dptr(do), _dptr(dc),
                 _stream_ptr(stream) if in_place else None)
    if in_place:
        return do, dc
    params.synchronize()
    return do.cpu().numpy(), int(dc.item())


def shamir_valid_mask(status=None, noise=None, *, status_bits: int = 0xFFFFFFFF, noise_bound: int = 0xFFFFFFFFFFFFFFFF,
                      host: bool = False, params: Optional[PvwParameters] = None, stream=None):
    """EXTENSION: the holder mask of a report.  status (uint32) and noise (uint64) are [rows][count] matrices (a
    vector is one row: the col_err of a corrected reconstruction; the [party][dealer] report of decrypt_all_party_shares_checked
    as it is); either may be None.  valid[c] = 1 iff no row has status & status_bits != 0 or noise > noise_bound in column c.
    Returns (valid uint8 [count], number of ones).  host=True: pvw_shamir_valid_mask_host.  Device tensors (int32 status, int64
    noise) are read in place on `stream` and (valid, count) stay on the device: what decrypt_all_party_handover takes."""
    if status is None and noise is None:
        raise PvwError(15, "status and noise are both None")
    if any(hasattr(a, "data_ptr") for a in (status, noise)):
        import torch
        first = status if status is not None else noise
        if params is None or host or any(a is not None and (not hasattr(a, "data_ptr") or not a.is_contiguous() or a.shape != first.shape)
                                         for a in (status, noise)) or first.dim() not in (1, 2):
            raise PvwError(15, "device reports need params, host=False and contiguous arrays of one shape")
        rows, count = (1, first.shape[0]) if first.dim() == 1 else tuple(first.shape)
        d_valid = torch.zeros(count, dtype=torch.uint8, device=first.device)
        d_num = torch.zeros(1, dtype=torch.int32, device=first.device)
        params._call("pvw_shamir_valid_mask_device", _dptr(status), _dptr(noise), int(status_bits), int(noise_bound), count, rows, count, 1,
                     _dptr(d_valid), _dptr(d_num), _stream_ptr(stream))
        return d_valid, d_num
    st = None if status is None else np.atleast_2d(np.ascontiguousarray(np.asarray(status, dtype=np.uint32)))
    nz = None if noise is None else np.atleast_2d(np.ascontiguousarray(np.asarray(noise).astype(np.uint64, copy=False)))
    shape = (st if st is not None else nz).shape
    if len(shape) != 2 or (st is not None and nz is not None and st.shape != nz.shape):
        raise PvwError(15, "status and noise must be arrays of one shape")
    rows, count = shape
    out, num = np.zeros(count, dtype=np.uint8), C.c_uint32()
    if host:
        L = params._lib if params is not None else _ffi.lib()
        _check(L.pvw_shamir_valid_mask_host(_ptr(st), _ptr(nz), int(status_bits), int(noise_bound), count, rows, count, 1, _ptr(out),
                                            C.byref(num)), L)
        return out, int(num.value)
    if params is None:
        raise PvwError(15, "the device form needs params (or host=True)")
    import torch
    d_st = torch.from_numpy(st.view(np.int32)).cuda() if st is not None else None
    d_nz = torch.from_numpy(nz.view(np.int64)).cuda() if nz is not None else None
    d_valid, d_num = torch.zeros(count, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    params._call("pvw_shamir_valid_mask_device", _dptr(d_st), _dptr(d_nz), int(status_bits), int(noise_bound), count, rows, count, 1,
                 _dptr(d_valid), _dptr(d_num), None)
    params.synchronize()
    return d_valid.cpu().numpy(), int(d_num.item())


def decrypt_all_party_handover(cts: Sequence[PvwCiphertext], parties: Sequence["Party"], indices: Sequence[int], plain_modulus: int,
                               valid=None, targets=None, wide: bool = False, *, bound: Optional[int] = None) -> CheckedDecryption:
    """EXTENSION: the handover of a one-word sharing in one call.  cts [D] are the old holders' re-dealt ciphertexts
    (holder d at party index indices[d]); targets as in shamir_handover_weights (None: the point 0; p - 1 - m, m < K, for a packed
    old sharing).  `valid` as a host array goes through pvw_decrypt_all_handover (only valid holders are uploaded); as a device
    tensor (uint8 [D]) it is used in place by pvw_decrypt_all_handover_device, read when the kernels run.  Returns the report
    [P][T] of decrypt_all_party_combinations_many: values[j][m] = sum_d lambda_{d,m} f_d(j + 1) mod p, new party j's share at
    target m; .count is the number of valid holders."""
    cts = list(cts)
    D = len(cts)
    p, repr, _ = _sum_inputs(cts, None)
    idx = _words(indices)
    if len(idx) != D:
        raise PvwError(15, f"indices: expected {D} holders, got {len(idx)}")
    v, dv = _holder_mask(valid, D)
    tg = None if targets is None else _words(targets)
    T, NP = (1 if tg is None else len(tg)), len(parties)
    lo = parties[0].index if NP else 0
    for i, party in enumerate(parties):
        if party.index != lo + i:
            raise PvwError(1, f"Party indices must be consecutive: {party.index} follows {lo + i - 1}")
    out, noise, status = np.zeros((NP, T), np.uint64), np.zeros((NP, T), np.uint64), np.zeros((NP, T), np.uint32)
    on, m, ww, wd = _plain(p, plain_modulus, wide, out.shape)
    count = C.c_uint32()
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2s = np.ascontiguousarray(np.stack([ct.c2 for ct in cts]), dtype=np.uint64)
    sk = np.ascontiguousarray(np.stack([_i64(party.secret_key.secret_coeffs) for party in parties])) if NP else np.zeros(1, np.int64)
    try:
        if dv is None:
            p._call("pvw_decrypt_all_handover", lo, lo + NP, _ptr(sk), _ptr(c1s), _ptr(c2s), D, _ptr(v), _ptr(idx), _ptr(tg), T, repr,
                    _ptr(out), _ptr(noise), _ptr(status), C.byref(count), m, ww, _ptr(wd))
            nv = int(count.value)
        else:
            import torch
            dev = dv.device
            up = lambda a: torch.from_numpy(a.view(np.int64)).to(dev)
            d_sk, d_c1, d_c2 = up(sk), up(c1s), up(c2s)
            d_out, d_noise = torch.zeros((NP, T), dtype=torch.int64, device=dev), torch.zeros((NP, T), dtype=torch.int64, device=dev)
            d_status, d_count = torch.zeros((NP, T), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            d_wide = torch.zeros((NP, T, ww), dtype=torch.int64, device=dev) if ww else None
            torch.cuda.synchronize(dev)
            try:
                p._call("pvw_decrypt_all_handover_device", lo, lo + NP, _dptr(d_sk), _dptr(d_c1), _dptr(d_c2), D, _dptr(dv), _ptr(idx),
                        _ptr(tg), T, repr, _dptr(d_out), _dptr(d_noise), _dptr(d_status), _dptr(d_count), m, ww, _dptr(d_wide), None)
                p.synchronize()
            finally:
                d_sk.zero_()
            out, noise = d_out.cpu().numpy().view(np.uint64), d_noise.cpu().numpy().view(np.uint64)
            status, nv = d_status.cpu().numpy().view(np.uint32), int(d_count.item())
            wd = d_wide.cpu().numpy().view(np.uint64) if ww else None
    finally:
        sk.fill(0)                                                         # the stacked copy of the keys (secret_key.rs:20-30)
    rep = CheckedDecryption(out, noise, status, _bound(p, bound), on, wd)
    rep.count = nv
    return rep


def _dptr(x):
    """a device buffer: a torch tensor (its data_ptr()), a raw address as an int, or None"""
    if x is None:
        return None
    return C.c_void_p(int(x.data_ptr() if hasattr(x, "data_ptr") else x) or None)


class DeviceSecretKey:
    """pvw_sk: a SecretKey's NTT form on the device (pvw_sk_load); cleared by free() / on drop (pvw_sk_free), as the
    reference's SecretKey is ZeroizeOnDrop (secret_key.rs:20-30).  Use as a context manager or call free()."""

    def __init__(self, secret_key: SecretKey):
        self.params = secret_key.params
        h = C.c_void_p()
        sk = _i64(secret_key.secret_coeffs)
        self.params._call("pvw_sk_load", _ptr(sk), C.byref(h))
        self._h = h

    @staticmethod
    def from_seed(params: "PvwParameters", seed: bytes, party_index: int) -> "DeviceSecretKey":
        """pvw_sk_load_seeded: the resident key of SecretKey.random(params, seed, party_index), drawn on the device -- the
        coefficients exist neither on the host nor in a device buffer."""
        key = DeviceSecretKey.__new__(DeviceSecretKey)
        key.params, key._h = params, None
        h = C.c_void_p()
        sd = _seed(seed)
        try:
            params._call("pvw_sk_load_seeded", _ptr(sd), int(party_index), C.byref(h))
        finally:
            sd.fill(0)
        key._h = h
        return key

    def free(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _check(_ffi.lib().pvw_sk_free(h))

    def decrypt_device_checked(self, d_c1s, d_c2col, num_dealers: int, d_noisy, d_out, d_noise=None, d_status=None,
                               stream=None, in_repr: int = REPR_NTT, *, plain_modulus: Optional[int] = None, wide=None,
                               wide_words: int = 0) -> None:
        """pvw_decrypt_batch_device_sk_checked: device buffers (torch tensors or raw addresses) -- d_out [D] the values,
        d_noise [D] uint64 and d_status [D] uint32 the report (either may be None); asynchronous on `stream`.
        plain_modulus / wide (a device buffer [D][wide_words]): pvw_decrypt_batch_device_sk_plain."""
        if not self._h:
            raise PvwError(1, "the DeviceSecretKey has been freed")
        if plain_modulus or wide is not None:
            self.params._call("pvw_decrypt_batch_device_sk_plain", self._h, _dptr(d_c1s), _dptr(d_c2col), int(num_dealers),
                              in_repr, _dptr(d_noisy), _dptr(d_out), _dptr(d_noise), _dptr(d_status), int(plain_modulus or 0),
                              int(wide_words), _dptr(wide), _stream_ptr(stream))
            return
        self.params._call("pvw_decrypt_batch_device_sk_checked", self._h, _dptr(d_c1s), _dptr(d_c2col), int(num_dealers),
                          in_repr, _dptr(d_noisy), _dptr(d_out), _dptr(d_noise), _dptr(d_status), _stream_ptr(stream))

    def decrypt_sum_device_checked(self, d_c1s, d_c2col, num_dealers: int, d_out, d_valid=None, d_noisy=None, d_noise=None,
                                   d_status=None, d_count=None, stream=None, in_repr: int = REPR_NTT, *,
                                   plain_modulus: Optional[int] = None, wide=None, wide_words: int = 0) -> None:
        """pvw_decrypt_sum_device_sk_checked: this party's aggregate share from ONE decrypt of the sum of the valid dealers'
        ciphertexts.  Device buffers: d_valid uint8 [D] (None = all), d_out / d_noise / d_status [1], d_count uint32 [1];
        asynchronous on `stream`.  plain_modulus / wide (a device buffer [wide_words]): pvw_decrypt_sum_device_sk_plain
        (DESIGN 8.8)."""
        if not self._h:
            raise PvwError(1, "the DeviceSecretKey has been freed")
        if plain_modulus or wide is not None:
            self.params._call("pvw_decrypt_sum_device_sk_plain", self._h, _dptr(d_c1s), _dptr(d_c2col), int(num_dealers),
                              _dptr(d_valid), in_repr, _dptr(d_noisy), _dptr(d_out), _dptr(d_noise), _dptr(d_status),
                              _dptr(d_count), int(plain_modulus or 0), int(wide_words), _dptr(wide), _stream_ptr(stream))
            return
        self.params._call("pvw_decrypt_sum_device_sk_checked", self._h, _dptr(d_c1s), _dptr(d_c2col), int(num_dealers),
                          _dptr(d_valid), in_repr, _dptr(d_noisy), _dptr(d_out), _dptr(d_noise), _dptr(d_status), _dptr(d_count),
                          _stream_ptr(stream))

    def decrypt_lincomb_device_plain(self, d_c1s, d_c2col, num_dealers: int, d_weights, d_out, d_valid=None, d_noisy=None,
                                     d_noise=None, d_status=None, d_count=None, stream=None, in_repr: int = REPR_NTT, *,
                                     plain_modulus: Optional[int] = None, wide=None, wide_words: int = 0) -> None:
        """pvw_decrypt_lincomb_device_sk_plain: this party's share of sum_d w_d m_d from ONE decrypt of the combination of the
        participating dealers' ciphertexts.  Device buffers: d_weights int64 [D], d_valid uint8 [D] (None = all), d_out /
        d_noise / d_status [1], d_count uint32 [1], wide [wide_words]; asynchronous on `stream`."""
        if not self._h:
            raise PvwError(1, "the DeviceSecretKey has been freed")
        self.params._call("pvw_decrypt_lincomb_device_sk_plain", self._h, _dptr(d_c1s), _dptr(d_c2col), int(num_dealers),
                          _dptr(d_valid), _dptr(d_weights), in_repr, _dptr(d_noisy), _dptr(d_out), _dptr(d_noise), _dptr(d_status),
                          _dptr(d_count), int(plain_modulus or 0), int(wide_words), _dptr(wide), _stream_ptr(stream))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _stream_ptr(stream):
    """a torch stream (its .cuda_stream), a raw hipStream_t as an int, or None (the state's own stream)"""
    if stream is None:
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None)


def sample_secret_keys_device(params: "PvwParameters", seed: bytes, party_lo: int, count: int, out=None, stream=None):
    """pvw_sample_secret_keys_device: the keys of parties [party_lo, party_lo + count) -- SecretKey.random(params, seed, p) each --
    drawn straight into a torch int64 tensor [count][k][l] on the device (`out`, or a new one), asynchronously on `stream`:
    what the d_sk argument of the *_device decrypt calls takes.  The tensor is key material; the caller clears it."""
    import torch
    if out is None:
        dev = torch.device("cuda", params.device) if getattr(params, "device", -1) >= 0 else torch.device("cuda")
        out = torch.empty((int(count), params.k, params.l), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != int(count) * params.k * params.l:
        raise PvwError(1, f"out must be a contiguous int64 tensor of {int(count) * params.k * params.l} elements")
    sd = _seed(seed)
    try:
        params._call("pvw_sample_secret_keys_device", _ptr(sd), int(party_lo), int(count), _dptr(out), _stream_ptr(stream))
    finally:
        sd.fill(0)
    return out


class DeviceRandomness:
    """pvw_rnd_state: a 32-byte seed S and a 64-bit counter c on the device.  Encrypts given `randomness=` (or the
    *_rs_device calls) read it when their kernels run and advance c themselves -- c + 1 per single encrypt, c + D per
    D-dealer encrypt -- so calls captured into a graph draw fresh randomness on every replay, as the reference's
    thread_rng() does on every encrypt (encryption.rs:135-167).  Calls on one stream at a time.  Freed (the device seed
    cleared first) by free(), on leaving a `with` block, or when dropped; always through the library that created it."""

    def __init__(self, params: "PvwParameters", seed: bytes, counter: int = 0):
        self.params = params                     # keeps the context (whose stream the state records) alive
        self._lib = params._lib
        self._h = None
        h = C.c_void_p()
        sd = _seed(seed)
        params._call("pvw_rnd_state_create", _ptr(sd), int(counter) & 0xFFFFFFFFFFFFFFFF, C.byref(h))
        sd.fill(0)
        self._h = h

    @staticmethod
    def call_seed(seed: bytes, counter: int) -> bytes:
        """call_seed(S, c): the seed a call that runs at counter c draws from (host only, no GPU)."""
        sd = _seed(seed)
        out = np.zeros(32, dtype=np.uint8)
        _check(_ffi.lib().pvw_rnd_call_seed(_ptr(sd), int(counter) & 0xFFFFFFFFFFFFFFFF, _ptr(out)))
        return out.tobytes()

    def _handle(self):
        if self._h is None:
            raise PvwError(1, "the DeviceRandomness has been freed")
        return self._h

    def counter(self, stream=None) -> int:
        """the counter once the work enqueued on `stream` (default: the context's stream) is done; waits for it"""
        v = C.c_uint64(0)
        _check(self._lib.pvw_rnd_state_counter(self._handle(), _stream_ptr(stream), C.byref(v)), self._lib)
        return int(v.value)

    def set_counter(self, counter: int, stream=None) -> None:
        """stream-ordered write of the counter"""
        _check(self._lib.pvw_rnd_state_set_counter(self._handle(), int(counter) & 0xFFFFFFFFFFFFFFFF, _stream_ptr(stream)),
               self._lib)

    def free(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _check(self._lib.pvw_rnd_state_free(h), self._lib)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _rnd_free_residue(lib=None) -> int:
    """SELF-TEST: seed words the calling thread's last DeviceRandomness.free() found not cleared (0 = cleared)"""
    v = C.c_uint64(0)
    _check((lib or _ffi.lib()).pvw_selftest_rnd_free_residue(C.byref(v)), lib)
    return int(v.value)


def _decrypt_batch(p, cts, secret_key, party_index, return_noisy=False):
    repr = cts[0].repr
    c1s = np.ascontiguousarray(np.stack([ct.c1 for ct in cts]), dtype=np.uint64)
    c2col = np.ascontiguousarray(np.stack([ct.c2[party_index] for ct in cts]), dtype=np.uint64)
    sk = _i64(secret_key.secret_coeffs)
    out = np.zeros(len(cts), dtype=np.uint64)
    noisy = np.zeros((len(cts), p.L, p.l), dtype=np.uint64) if return_noisy else None
    p._call("pvw_decrypt_batch", _ptr(sk), _ptr(c1s), _ptr(c2col), len(cts), repr,
                                        _ptr(out), _ptr(noisy))
    vals = [int(v) for v in out]
    return (vals, noisy) if return_noisy else vals


def decrypt_party_value(ciphertext: PvwCiphertext, secret_key: SecretKey, party_index: int) -> int:
    """decrypt_party_value (decryption.rs:249-278)."""
    return _decrypt_batch(ciphertext.params, [ciphertext], secret_key, party_index)[0]


def _secret_residue(params: PvwParameters) -> Tuple[int, int]:
    """(non-zero words, scanned words) of the device regions the last key-bearing calls declared secret."""
    nz, sc = C.c_uint64(), C.c_uint64()
    params._call("pvw_selftest_secret_residue", C.byref(nz), C.byref(sc))
    return nz.value, sc.value


def _selftest_decode_fixed(params: PvwParameters, noisy: np.ndarray) -> List[int]:
    """Host run of the fixed-width decode the GPU executes (self-test hook, see pvw_hip.h)."""
    a = _u64(noisy).reshape(-1, params.L, params.l)
    out = np.zeros(len(a), dtype=np.uint64)
    params._call("pvw_selftest_decode_fixed", _ptr(a), len(a), _ptr(out))
    return [int(v) for v in out]


def decode_scalar_pvw(params: PvwParameters, noisy: np.ndarray) -> List[int]:
    """decode_scalar_pvw_rns (decryption.rs:10-58) on power-basis noisy polynomials [D][L][l], on the device."""
    a = _u64(noisy).reshape(-1, params.L, params.l)
    out = np.zeros(len(a), dtype=np.uint64)
    params._call("pvw_decode", _ptr(a), len(a), _ptr(out))
    return [int(v) for v in out]


def decode_scalar_pvw_host(params: PvwParameters, noisy: np.ndarray) -> List[int]:
    """The same decode with host big integers (no GPU): cross-check of the device algorithm."""
    a = _u64(noisy).reshape(-1, params.L, params.l)
    out = np.zeros(len(a), dtype=np.uint64)
    params._call("pvw_decode_host", _ptr(a), len(a), _ptr(out))
    return [int(v) for v in out]


def _decode_checked(params: PvwParameters, noisy, fn: str, bound) -> CheckedDecryption:
    a = _u64(noisy).reshape(-1, params.L, params.l)
    out = np.zeros(len(a), dtype=np.uint64)
    noise = np.zeros(len(a), dtype=np.uint64)
    status = np.zeros(len(a), dtype=np.uint32)
    params._call(fn, _ptr(a), len(a), _ptr(out), _ptr(noise), _ptr(status))
    return CheckedDecryption(out, noise, status, _bound(params, bound))


def decode_scalar_pvw_checked(params: PvwParameters, noisy: np.ndarray, bound: Optional[int] = None) -> CheckedDecryption:
    """decode_scalar_pvw with each polynomial's report (pvw_decode_checked, on the device)."""
    return _decode_checked(params, noisy, "pvw_decode_checked", bound)


def decode_scalar_pvw_checked_host(params: PvwParameters, noisy: np.ndarray, bound: Optional[int] = None) -> CheckedDecryption:
    """The same with host big integers, residuals by their definition (pvw_decode_checked_host; no GPU)."""
    return _decode_checked(params, noisy, "pvw_decode_checked_host", bound)


def _selftest_decode_checked(params: PvwParameters, noisy: np.ndarray) -> CheckedDecryption:
    """Host run of the fixed-width device decode with its report (self-test hook, see pvw_hip.h)."""
    return _decode_checked(params, noisy, "pvw_selftest_decode_checked", 0)


def _decode_plain(params: PvwParameters, noisy, fn: str, bound, plain_modulus, wide_words) -> CheckedDecryption:
    """the plain decode of [count][L][l] polynomials: wide_words None = every word of Q, 0 = none"""
    a = _u64(noisy).reshape(-1, params.L, params.l)
    out = np.zeros(len(a), dtype=np.uint64)
    noise = np.zeros(len(a), dtype=np.uint64)
    status = np.zeros(len(a), dtype=np.uint32)
    m = int(plain_modulus or 0)
    ww = (params.q_total().bit_length() + 63) // 64 if wide_words is None else int(wide_words)
    wd = np.zeros((len(a), ww), dtype=np.uint64) if ww else None
    params._call(fn, _ptr(a), len(a), _ptr(out), _ptr(noise), _ptr(status), m, ww, _ptr(wd))
    return CheckedDecryption(out, noise, status, _bound(params, bound), bool(m or ww), wd)


def decode_scalar_pvw_plain(params: PvwParameters, noisy: np.ndarray, plain_modulus: Optional[int] = None, wide_words: Optional[int] = 0,
                            bound: Optional[int] = None) -> CheckedDecryption:
    """decode_scalar_pvw_checked finished in the caller's modulus and / or as wide integers (pvw_decode_plain, on the device)."""
    return _decode_plain(params, noisy, "pvw_decode_plain", bound, plain_modulus, wide_words)


def decode_scalar_pvw_plain_host(params: PvwParameters, noisy: np.ndarray, plain_modulus: Optional[int] = None,
                                 wide_words: Optional[int] = 0, bound: Optional[int] = None) -> CheckedDecryption:
    """The same with host big integers, by the definition (pvw_decode_plain_host; no GPU)."""
    return _decode_plain(params, noisy, "pvw_decode_plain_host", bound, plain_modulus, wide_words)


def _selftest_decode_plain(params: PvwParameters, noisy: np.ndarray, plain_modulus=None, wide_words=0) -> CheckedDecryption:
    """Host run of the fixed-width device decode with the plain tail (self-test hook, see pvw_hip.h)."""
    return _decode_plain(params, noisy, "pvw_selftest_decode_plain", 0, plain_modulus, wide_words)


# ---- wire format, version 1 ----
_WIRE_MAGIC = b"PVWw"
_WIRE_FIXED = 48                     # header bytes before the moduli


def _wire_header(p: PvwParameters, kind: int, repr: int = REPR_POWER, lo: int = 0, hi: int = 0, lo2: int = 0, hi2: int = 0) -> np.ndarray:
    n = C.c_size_t()
    p._call("pvw_wire_header", kind, repr, lo, hi, lo2, hi2, None, 0, C.byref(n))
    buf = np.zeros(n.value, dtype=np.uint8)
    p._call("pvw_wire_header", kind, repr, lo, hi, lo2, hi2, _ptr(buf), n.value, C.byref(n))
    return buf


def _wire_check(p: PvwParameters, data, kind: int):
    """pvw_wire_header_check on a whole blob, which must be of `kind`: (repr, ranges, header length, the blob as uint8)"""
    a = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)[:0]
    kd, rp, hl = C.c_uint32(), C.c_uint32(), C.c_size_t()
    rg = (C.c_uint32 * 4)()
    buf = a if len(a) else np.zeros(1, dtype=np.uint8)
    p._call("pvw_wire_header_check", _ptr(buf), len(a), C.byref(kd), C.byref(rp), rg, C.byref(hl))
    if kd.value != kind:
        raise PvwError(18, f"wire: the blob is of kind {kd.value}, expected kind {kind}")
    return rp.value, tuple(int(x) for x in rg), int(hl.value), a


def wire_pack_host(params: PvwParameters, polys) -> bytes:
    """the format's packing of polynomials [..][L][l] in plain C++ on the host (pvw_wire_pack_host)"""
    a = _u64(polys)
    count = a.size // (params.L * params.l)
    out = np.zeros(count * params.wire_poly_bytes() + 1, dtype=np.uint8)
    params._call("pvw_wire_pack_host", _ptr(a), count, _ptr(out))
    return out[:-1].tobytes()


def wire_unpack_host(params: PvwParameters, data, count: int) -> np.ndarray:
    """pvw_wire_unpack_host: DeserializationError naming the first residue >= q_i"""
    a = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    out = np.zeros((count, params.L, params.l), dtype=np.uint64)
    bad = C.c_uint64()
    params._call("pvw_wire_unpack_host", _ptr(a), count, _ptr(out), C.byref(bad))
    return out


def wire_pack(params: PvwParameters, polys) -> bytes:
    """pvw_wire_pack: packed on the device"""
    a = _u64(polys)
    count = a.size // (params.L * params.l)
    out = np.zeros(count * params.wire_poly_bytes() + 1, dtype=np.uint8)
    params._call("pvw_wire_pack", _ptr(a), count, _ptr(out))
    return out[:-1].tobytes()


def wire_unpack(params: PvwParameters, data, count: int) -> np.ndarray:
    """pvw_wire_unpack: unpacked and checked on the device"""
    a = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    out = np.zeros((count, params.L, params.l), dtype=np.uint64)
    params._call("pvw_wire_unpack", _ptr(a), count, _ptr(out))
    return out

"""GPU checks at the modulus widths the kernels branch on (tests/_util.py MOD_CLASSES / EDGE_CHAINS), bit for bit against
the C oracle or the big-integer model: transforms, keygen, single- and multi-dealer encrypt, the decrypt inner products,
decrypt_all and the device decode.  The CPU side (the arithmetic, the checker itself) is tests/test_modulus_edges_host.py.

The API does not say which kernel form ran; the routing rules each case exercises are stated where the case is built:
  - packed mac_rows stream (single-dealer encrypt): widest modulus <= 40 / 48 / 56 bits and k % 64 == 0 -> 40 / 48 / 56,
    <= 61 bits and k % 256 == 0 -> 61, else unpacked (packed_width; what packed_active() reports)
  - digit GEMM contraction: keygen (>= 8 parties) and decrypt_all (>= 22 parties) always contract 8 bytes; encrypt_many
    (>= 3 dealers) contracts 7 when the widest modulus <= 56 bits and k % 64 == 0 (gemm7_ok: vec_digits7_kernel,
    mftile7_kernel), else 8 -- mixed_tiny_among_56 / mixed_above256_among_56 carry q = 241 / 257 through the 7-byte form
    (whose seven digit-step values stayed congruent and below 2^56 even with the old w = 256 constants, so its results
    were exact before the fix too: which constants it uses is checked on the host, test_modulus_edges_host.py)
  - digit GEMM recombination: f64 quotient estimate (FASTQ) when the smallest modulus >= 55 bits; biased f64 form when
    k <= 512, signed integer form above
  - digit step of the GEMM operands (vec_digits*_kernel): Shoup multiply by 256 mod q (mul256_consts), q < 256 included"""
import numpy as np
import pytest

import pvw_model as M
import pvw_oracle as O
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import EDGE_CHAINS, MIXED_CHAINS, PURE_CHAINS, SEED, chain_max_l, primes_1mod, rns_to_ring
import test_gpu_decrypt_all as DA
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

CHAINS = sorted(EDGE_CHAINS)
# encrypt checks the reference's correctness gate: the pure tiny / just-above-256 chains fail it at every geometry here
# (Delta^(l-1) of 17 and 14 bits), so those classes are encrypted only inside the mixed chains tiny_* / above256_*
ENCRYPT_CHAINS = [c for c in CHAINS if c not in ("pure_tiny", "pure_above256")]
# the packed stream width single-dealer encrypt must pick at (n, k, l) = (40, 256, 8): widest modulus 32..40 bits -> 40,
# 41..48 -> 48, 49..56 -> 56, 57..61 -> 61, 62 -> none
PACKED_WIDTH = {
    "pure_around32": 40, "pure_top40": 40, "pure_bottom48": 48, "pure_bottom56": 56, "pure_top54": 56, "pure_bottom55": 56,
    "pure_top56": 56, "pure_bottom57": 61, "pure_bottom62": 0, "pure_top62": 0,
    "mixed_tiny_first": 61, "mixed_tiny_last": 61, "mixed_tiny_all": 61, "mixed_above256_first": 61,
    "mixed_top54_among_61": 61, "mixed_bottom57_among_top56": 61, "mixed_top62_among_40": 0,
    "mixed_tiny_among_56": 56, "mixed_above256_among_56": 56,
}
# the FASTQ line (smallest modulus 54 | 55 bits) and the 62-bit chains, with the tiny-q_0 chain: keygen at k > 512 as well
WIDE_K_CHAINS = ["pure_top54", "pure_bottom55", "pure_bottom62", "pure_top62", "mixed_top54_among_61", "mixed_tiny_first"]


def test_every_encrypt_chain_passes_the_gate():
    assert sorted(PACKED_WIDTH) == ENCRYPT_CHAINS
    for name in ENCRYPT_CHAINS:
        for n, k in ((40, 256), (20, 576), (64, 256), (40, 512)):
            assert T.build_params(n, k, 8, EDGE_CHAINS[name]).verify_correctness_condition(), (name, n, k)


@pytest.mark.parametrize("name", CHAINS)
def test_ntt_round_trip_and_oracle(name):
    # ntt_forward / ntt_inverse / from_coefficients (INT64_MIN / MAX among the coefficients) against the oracle, at l = 8 and
    # the largest l the chain serves
    moduli = EDGE_CHAINS[name]
    for l in sorted({8, chain_max_l(moduli)}):
        T.test_ntt_round_trip_and_oracle(l, moduli)


# (n, k): 5 parties -> integer VALU; 40 -> GEMM streaming the transposed CRS; 70 -> GEMM with the parties as rows
@pytest.mark.parametrize("n,k", [(5, 12), (40, 24), (70, 12)])
@pytest.mark.parametrize("name", CHAINS)
def test_keygen_against_c_oracle(name, n, k):
    T.batched_keygen_case(n, k, 8, None, EDGE_CHAINS[name])


# k = 256: biased f64 recombination; k = 528: signed integer recombination (both with FASTQ or not by the chain's
# smallest modulus; keygen contracts 8 bytes at every k)
@pytest.mark.parametrize("n,k", [(40, 256), (70, 528)])
@pytest.mark.parametrize("name", WIDE_K_CHAINS)
def test_keygen_wide_k_against_c_oracle(name, n, k):
    T.batched_keygen_case(n, k, 8, None, EDGE_CHAINS[name])


@pytest.mark.parametrize("name", ENCRYPT_CHAINS)
def test_single_dealer_encrypt_at_the_stream_width(name):
    # (40, 256, 8) qualifies for a packed stream at every width; (9, 40, 8) for none (k % 64 != 0)
    run, c1o, c2o = T.mac_rows_case(40, 256, 8, None, EDGE_CHAINS[name])
    for _ in range(2):
        ct = run()
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
        assert run.params.packed_active() == PACKED_WIDTH[name]
    run, c1o, c2o = T.mac_rows_case(9, 40, 8, None, EDGE_CHAINS[name])
    ct = run()
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    assert run.params.packed_active() == 0


# D = 2: integer VALU; D = 5, 40: digit GEMM.  k = 256: biased recombination, 7-byte contraction where every modulus is
# <= 56 bits (pure_around32 .. pure_top56, mixed_tiny_among_56, mixed_above256_among_56); k = 576: signed integer
# recombination, 7 bytes likewise (576 % 64 == 0)
@pytest.mark.parametrize("k,D", [(256, 2), (256, 5), (256, 40), (576, 5), (576, 40)])
@pytest.mark.parametrize("name", ENCRYPT_CHAINS)
def test_encrypt_many_equals_separate_encrypts_and_oracle(name, k, D):
    T.digit_gemm_case(20, k, 8, EDGE_CHAINS[name], D)


EXTREME_CHAINS = ["pure_top56", "pure_bottom62", "pure_top62", "mixed_bottom57_among_top56"]


@pytest.mark.parametrize("n,k,D", [(64, 256, 20), (40, 512, 17)])
@pytest.mark.parametrize("name", EXTREME_CHAINS)
def test_digit_gemm_extreme_matrix_bytes(name, n, k, D):
    # byte 6 of the top-of-56 residues up to 0xff in the 7-byte form; 62-bit residues (q close to 2^62) in the 8-byte form
    T.digit_gemm_extreme_case(n, k, 8, EDGE_CHAINS[name], D)


@pytest.fixture
def tuning_library():
    prev = _ffi.select("tuning")
    yield
    _ffi.select(prev)


@pytest.mark.parametrize("k,D", [(256, 5), (576, 40)])
@pytest.mark.parametrize("name", ["pure_top56", "pure_bottom56"])
def test_top_of_56_through_the_eight_byte_contraction(name, k, D, tuning_library, monkeypatch):
    # PVW_GEMM_BYTES=8 (tuning build): the same 56-bit chains through the general 8-byte contraction
    monkeypatch.setenv("PVW_GEMM_BYTES", "8")
    T.digit_gemm_case(20, k, 8, EDGE_CHAINS[name], D)


# (k, D): one full wave of slot pairs and a remainder at L = 2..5; k = 300 cuts the inner products into ragged ranges
@pytest.mark.parametrize("k,D", [(20, 9), (300, 4)])
@pytest.mark.parametrize("name", CHAINS)
def test_decrypt_batch_against_oracle_and_model(name, k, D):
    moduli = EDGE_CHAINS[name]
    run, want = T.decrypt_mac_case(k, 8, None, D, moduli)
    assert np.array_equal(run(), want)
    # the decoded values of ciphertext-shaped noisy polynomials: c2 = <sk, c1> - m Delta^j + noise
    p = T.build_params(3, k, 8, moduli)
    m = M.Params(3, k, 8, moduli)
    orc = O.Oracle(moduli, 8)
    L = len(moduli)
    c1s = orc.fill_uniform(SEED, M.DOM_CRS, 1, D * k).reshape(D, k, L, 8)
    sk = O.sample_cbd(SEED, M.DOM_SK, 1, k, 8, 0.5)
    inner = orc.decrypt_noisy(sk, c1s, np.zeros((D, L, 8), dtype=np.uint64))   # <sk, c1>, power basis
    rng = np.random.default_rng(k + D)
    msgs = [int(x) for x in rng.integers(0, 1 << 63, size=D)]
    msgs[0] = (1 << 64) - 1
    ring = [[-(msg * m.delta ** j) + int(e) for j, e in enumerate(rng.integers(-40, 41, size=8))] for msg in msgs]
    enc = np.array([[[c % q for c in z] for q in moduli] for z in ring], dtype=np.uint64)
    qs = np.array(moduli, dtype=np.uint64)[None, :, None]
    c2 = orc.ntt_forward((inner + (qs - enc)) % qs)              # noisy = <sk, c1> - c2 = enc
    cts = [P.PvwCiphertext(c1s[d], np.repeat(c2[d][None], 3, axis=0), p, P.REPR_NTT) for d in range(D)]
    key = P.SecretKey.from_coefficients(p, sk)
    vals, noisy = P.api._decrypt_batch(p, cts, key, 0, return_noisy=True)
    assert np.array_equal(noisy, enc)
    want_vals = [M.decode_scalar_pvw(rns_to_ring(enc[d], moduli), m) for d in range(D)]
    assert [int(v) for v in vals] == want_vals


# 8 parties: the per-party kernels; 30: the digit GEMM over all parties, 8-byte contraction (the switch is at 22)
@pytest.mark.parametrize("hi", [10, 32])
@pytest.mark.parametrize("name", CHAINS)
def test_decrypt_all_against_per_party_and_oracle(name, hi):
    moduli = EDGE_CHAINS[name]
    n, k, l, lo, D = 40, 16, 8, 2, 6
    p = DA._params(n, k, l, moduli)
    m = M.Params(n, k, l, moduli)
    orc = O.Oracle(moduli, l)
    sk, c1, c2 = DA._random_inputs(p, lo, hi, D, seed=hi * 100 + len(moduli))
    got = DA._all(p, lo, hi, sk, c1, c2)
    DA._check_against_per_party(p, lo, hi, sk, c1, c2, got)
    for i in sorted({0, (hi - lo) // 2, hi - lo - 1}):
        noisy = orc.decrypt_noisy(sk[i], c1, c2[:, lo + i])
        want = [M.decode_scalar_pvw(rns_to_ring(noisy[d], moduli), m) for d in range(D)]
        assert [int(v) for v in got[i]] == want, i
    assert DA._residue(p)[0] == 0


DECODE_CHAINS = ([(8, MIXED_CHAINS[c], "mixed_" + c) for c in sorted(MIXED_CHAINS)]
                 + [(8, PURE_CHAINS[c], "pure_" + c) for c in ("tiny", "above256")]
                 + [(l, PURE_CHAINS[c], "pure_" + c) for c in ("bottom62", "top62") for l in (8, 16)]
                 + [(64, [257] + primes_1mod(128, 2), "257_l64")])


@pytest.mark.parametrize("l,moduli", [(l, m) for l, m, _ in DECODE_CHAINS], ids=[i for _, _, i in DECODE_CHAINS])
def test_device_decode_matches_model(l, moduli):
    T.device_decode_case(l, moduli, lambda variant: None, (0,))

"""The residue-word contract (include/pvw_hip.h) on the GPU: a word w a caller passes in limb i means w mod q_i, every
residue the library returns is below q_i (except NTT-domain downloads of an NTT-domain load: the stored words as given),
and signed inputs mean their signed residue (parameters.rs:440-443).  Every case runs the HIP path on RAW words and
compares it with the C oracle on the same words reduced in numpy (and, where one exists, the HIP path on the reduced
words): CRS and public keys into encrypt (single dealer, packed and unpacked streams; multi-dealer on the VALU, the 8-byte
and the 7-byte digit GEMM), key generation and the downloads; ciphertexts into every decrypt form, per party and for all
parties, host and device pointers; polynomials into the transforms; noisy residues into the decode."""
import ctypes as C

import numpy as np
import pytest

import pvw_model as M
import pvw_oracle as O
import pvw_rs_amd as P
from _util import EXAMPLE_MODULI, MIXED_CHAINS, MOD_TOP_62, SEED, TEST_MODULI, primes_1mod

pytestmark = pytest.mark.gpu

MAXW = (1 << 64) - 1
# chains: 56 bits (7-byte GEMM, 56-bit packed stream), 61 bits (8-byte GEMM, packed61), 37 bits (packed40), 62 bits
# (unpacked), and 241 among top-of-56 moduli (q < 2^9 on the 7-byte form)
CHAINS = {
    "example56": EXAMPLE_MODULI,
    "bench61": M.bench_moduli(2),
    "test40": TEST_MODULI,
    "top62": MOD_TOP_62,
    "tiny_among_56": MIXED_CHAINS["tiny_among_56"],
}
I64_EXTREMES = [-(1 << 63), (1 << 63) - 1, 1 << 62, -(1 << 62)]


def _params(n, k, l, moduli, bounds=(100, 200)):
    return (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
            .set_error_bounds(*bounds).build())


def class_words(q, w):
    """the unreduced word classes of limb q (w: a residue of that limb)"""
    t = (MAXW - w) // q
    out = [q - 1, q, w + q, w + t * q, (1 << 56) - 1, 1 << 56, 1 << 61, 1 << 62, (1 << 63) - (1 << 55) - 1,
           (1 << 63) - (1 << 55), 1 << 63, (1 << 64) - q, MAXW]
    if 2 * q - 1 <= MAXW:
        out.append(2 * q - 1)
    return out


def unreduced(red, moduli, seed, classes=True):
    """raw words for the reduced residues `red` [..][L][l]: most polynomials w + t q (t random, up to the largest that
    fits), every 5th polynomial the word classes over its slots (classes=True), polynomial 1 all w + t_max q, some left
    reduced.  Returns (raw, raw mod q) -- the class words change the residue, so the reduced copy is taken from raw."""
    rng = np.random.default_rng(seed)
    L, l = red.shape[-2], red.shape[-1]
    q = np.array(moduli, dtype=np.uint64)[:, None]
    tmax = (np.uint64(MAXW) - red) // q
    t = rng.integers(0, 1 << 62, size=red.shape, dtype=np.uint64) % (tmax + np.uint64(1))
    raw = (red + t * q).reshape(-1, L, l)
    rf, tf = red.reshape(-1, L, l), tmax.reshape(-1, L, l)
    keep = rng.random(raw.shape[0]) < 0.2
    raw[keep] = rf[keep]
    if raw.shape[0] > 1:
        raw[1] = rf[1] + tf[1] * q
    for i in range(0, raw.shape[0] if classes else 0, 5):
        for li, qq in enumerate(moduli):
            cls = class_words(qq, int(rf[i, li, 0]))
            for s in range(l):
                raw[i, li, s] = np.uint64(cls[(i // 5 + s + 3 * li) % len(cls)])
    raw = raw.reshape(red.shape)
    return raw, raw % q


def _below_q(a, moduli):
    return bool((a < np.array(moduli, dtype=np.uint64)[:, None]).all())


def _uniform(moduli, shape, seed):
    rng = np.random.default_rng(seed)
    q = np.array(moduli, dtype=np.uint64)[:, None]
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) % q


def _oracle_randomness(seed, n, k, l):
    return (O.sample_cbd(seed, M.DOM_R, 0, k, l, 0.5), O.sample_uniform(seed, M.DOM_E1, 0, k, l, 100),
            O.sample_uniform(seed, M.DOM_E2, 0, n, l, 200))


def _load_raw_system(p, moduli, repr, seed):
    """CRS and public key loaded from raw words in `repr`; returns (crs, gpk, a_hat, b_hat, a_raw, b_raw) with the NTT-domain
    residues the oracle works on"""
    n, k, l, L = p.n, p.k, p.l, p.L
    orc = O.Oracle(moduli, l)
    a_raw, a_red = unreduced(_uniform(moduli, (k, k, L, l), seed), moduli, seed + 1)
    b_raw, b_red = unreduced(_uniform(moduli, (n, k, L, l), seed + 2), moduli, seed + 3)
    crs = P.PvwCrs.from_polynomials(p, a_raw, repr)
    gpk = P.GlobalPublicKey.new(crs)
    gpk.load_rows(0, b_raw, repr)
    if repr == P.REPR_POWER:
        a_hat, b_hat = orc.ntt_forward(a_red), orc.ntt_forward(b_red)
    else:
        a_hat, b_hat = a_red, b_red
    return crs, gpk, a_hat, b_hat, a_raw, b_raw


def _check_downloads(p, moduli, repr, crs, gpk, a_hat, b_hat, a_raw, b_raw):
    orc = O.Oracle(moduli, p.l)
    for got, hat, raw in ((crs.matrix(P.REPR_NTT), a_hat, a_raw), (gpk.matrix(repr=P.REPR_NTT), b_hat, b_raw)):
        if repr == P.REPR_NTT:
            assert np.array_equal(got, raw)                     # the exception: an NTT-domain load comes back as given
        else:
            assert np.array_equal(got, hat) and _below_q(got, moduli)
    for got, hat in ((crs.matrix(P.REPR_POWER), a_hat), (gpk.matrix(repr=P.REPR_POWER), b_hat)):
        assert _below_q(got, moduli)
        assert np.array_equal(got, orc.ntt_inverse(hat))


# ------------------------------------------------------------------------------------------- CRS and public key
# (chain, n, k, l, dealer counts): k a multiple of 256 where the 61-bit packed stream needs it, 64 elsewhere
ENCRYPT_CASES = [
    ("example56", 24, 64, 8, (2, 3, 9)),
    ("bench61", 24, 256, 8, (2, 5)),
    ("test40", 20, 64, 16, (2, 4)),
    ("top62", 12, 64, 8, (2, 3)),
    ("tiny_among_56", 12, 64, 8, (2, 4)),
]


@pytest.mark.parametrize("repr", [P.REPR_NTT, P.REPR_POWER], ids=["ntt", "power"])
@pytest.mark.parametrize("chain,n,k,l,dealers", ENCRYPT_CASES, ids=[c[0] for c in ENCRYPT_CASES])
def test_raw_crs_and_public_key_into_encrypt_and_downloads(chain, n, k, l, dealers, repr):
    moduli = CHAINS[chain]
    p = _params(n, k, l, moduli)
    crs, gpk, a_hat, b_hat, a_raw, b_raw = _load_raw_system(p, moduli, repr, seed=n + k + repr)
    _check_downloads(p, moduli, repr, crs, gpk, a_hat, b_hat, a_raw, b_raw)
    orc = O.Oracle(moduli, l)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    scalars = np.array([(i * 7919 + 3) % (1 << 32) for i in range(n)], dtype=np.uint64)
    # single dealer (the packed stream where the geometry has one and the words fit it, else the tiled matrices)
    ct = P.encrypt(scalars, gpk, SEED)
    c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, scalars, *_oracle_randomness(SEED, n, k, l))
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    # multi-dealer: 2 dealers on the VALU, 3+ on the digit GEMM (7 bytes on chains <= 56 bits; e2 fused into its finish)
    for D in dealers:
        rows = [[(d * 104729 + i * 31 + 1) % (1 << 32) for i in range(n)] for d in range(D)]
        seeds = [P.api._dealer_seed(SEED, d) for d in range(D)]
        many = P.encrypt_many(rows, gpk, seeds)
        for d in sorted({0, D - 1}):
            c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(rows[d], dtype=np.uint64), *_oracle_randomness(seeds[d], n, k, l))
            assert np.array_equal(many[d].c1, c1o), f"c1 D={D} dealer {d}"
            assert np.array_equal(many[d].c2, c2o), f"c2 D={D} dealer {d}"
    # pvw_prepare built the derived copies (packed stream, MFMA tiles) from this key; then a DIFFERENT raw key is loaded and
    # used without another prepare: nothing derived from the first key may be read
    p.prepare()
    D = dealers[-1]
    rows = [[(d * 13 + i) % (1 << 32) for i in range(n)] for d in range(D)]
    seeds = [P.api._dealer_seed(bytes([7]) * 32, d) for d in range(D)]
    b2_raw, b2_red = unreduced(_uniform(moduli, (n, k, p.L, l), n + 77), moduli, n + 78)
    b2_hat = b2_red if repr == P.REPR_NTT else orc.ntt_forward(b2_red)
    for key, bh in (("prepared", b_hat), ("reloaded", b2_hat)):
        if key == "reloaded":
            gpk.load_rows(0, b2_raw, repr)
        ct = P.encrypt(scalars, gpk, SEED)
        c1o, c2o = orc.encrypt(a_hat, bh, g_hat, scalars, *_oracle_randomness(SEED, n, k, l))
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o), key
        many = P.encrypt_many(rows, gpk, seeds)
        for d in (0, D - 1):
            c1o, c2o = orc.encrypt(a_hat, bh, g_hat, np.array(rows[d], dtype=np.uint64), *_oracle_randomness(seeds[d], n, k, l))
            assert np.array_equal(many[d].c1, c1o) and np.array_equal(many[d].c2, c2o), f"{key}: dealer {d}"


def test_raw_words_give_what_the_reduced_words_give():
    # HIP on raw words against HIP on the same words reduced (a second context), for every encrypt form
    n, k, l, moduli = 24, 64, 8, EXAMPLE_MODULI
    outs = []
    for raw in (True, False):
        p = _params(n, k, l, moduli)
        a_raw, a_red = unreduced(_uniform(moduli, (k, k, 4, l), 5), moduli, 6)
        b_raw, b_red = unreduced(_uniform(moduli, (n, k, 4, l), 7), moduli, 8)
        gpk = P.GlobalPublicKey.new(P.PvwCrs.from_polynomials(p, a_raw if raw else a_red, P.REPR_NTT))
        gpk.load_rows(0, b_raw if raw else b_red, P.REPR_NTT)
        rows = [[(d * 3 + i) % (1 << 32) for i in range(n)] for d in range(9)]
        seeds = [P.api._dealer_seed(SEED, d) for d in range(9)]
        res = [P.encrypt(rows[0], gpk, SEED)]
        assert p.packed_active() == (0 if raw else 56)                # raw words do not fit the packed stream
        res += P.encrypt_many(rows[:2], gpk, seeds[:2]) + P.encrypt_many(rows, gpk, seeds)
        outs.append([(c.c1, c.c2) for c in res])
    for (a1, a2), (b1, b2) in zip(*outs):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)


# (chain, n, k, l): 64+ parties take the default matrix-core form, which digitises the columns of A-hat as stored
# (keygen_gemm_swapped: balanced 8-byte digits of every CRS word); 8..63 parties the transposed-CRS form (A^T as the raw
# 8-byte operand of the digit GEMM), fewer the VALU form, l = 64 through API-layout rows
KEYGEN_CASES = [
    ("bench61", 64, 64, 8), ("example56", 64, 64, 8), ("tiny_among_56", 70, 64, 8), ("test40", 64, 32, 16),
    ("bench61", 40, 64, 8), ("example56", 12, 64, 8), ("tiny_among_56", 5, 64, 8), ("top62", 9, 16, 64),
]


@pytest.mark.parametrize("chain,n,k,l", KEYGEN_CASES, ids=[f"{c[0]}-n{c[1]}" for c in KEYGEN_CASES])
def test_keygen_on_a_raw_crs(chain, n, k, l):
    # every key-generation form on a CRS of raw words, in both load representations, against the oracle on the reduced
    # words; sk / ek at the signed extremes in a few places
    moduli = CHAINS[chain]
    L = len(moduli)
    p = _params(n, k, l, moduli)
    orc = O.Oracle(moduli, l)
    for repr in (P.REPR_NTT, P.REPR_POWER):
        a_raw, a_red = unreduced(_uniform(moduli, (k, k, L, l), k + repr), moduli, l + repr)
        a_hat = a_red if repr == P.REPR_NTT else orc.ntt_forward(a_red)
        gpk = P.GlobalPublicKey.new(P.PvwCrs.from_polynomials(p, a_raw, repr))
        rng = np.random.default_rng(n)
        sk = rng.integers(-1, 2, size=(n, k, l), dtype=np.int64)
        ek = rng.integers(-100, 101, size=(n, k, l), dtype=np.int64)
        for i, v in enumerate(I64_EXTREMES + [moduli[0], -moduli[0]]):
            sk[i % n, i % k, i % l] = v
            ek[(i + 1) % n, (2 * i) % k, (3 * i) % l] = v
        gpk.generate_with_errors(0, sk, ek)
        got = gpk.matrix(repr=P.REPR_NTT)
        assert _below_q(got, moduli)
        assert np.array_equal(got, orc.keygen(a_hat, sk, ek)), f"repr {repr}"


# ------------------------------------------------------------------------------------------- ciphertexts
def _decrypt_batch(p, sk, c1, c2col, repr):
    out = np.zeros(c1.shape[0], dtype=np.uint64)
    nz = np.zeros((c1.shape[0], p.L, p.l), dtype=np.uint64)
    sk, c1, c2col = np.ascontiguousarray(sk), np.ascontiguousarray(c1), np.ascontiguousarray(c2col)
    p._call("pvw_decrypt_batch", sk.ctypes.data, c1.ctypes.data, c2col.ctypes.data, c1.shape[0], repr, out.ctypes.data,
            nz.ctypes.data)
    return out, nz


def _decrypt_all(p, lo, hi, sk, c1, c2, repr):
    out = np.zeros((hi - lo, c1.shape[0]), dtype=np.uint64)
    sk, c1, c2 = np.ascontiguousarray(sk), np.ascontiguousarray(c1), np.ascontiguousarray(c2)
    p._call("pvw_decrypt_all", lo, hi, sk.ctypes.data, c1.ctypes.data, c2.ctypes.data, c1.shape[0], repr, out.ctypes.data)
    return out


def _decode_host(p, noisy):
    out = np.zeros(noisy.shape[0], dtype=np.uint64)
    noisy = np.ascontiguousarray(noisy)
    p._call("pvw_decode_host", noisy.ctypes.data, noisy.shape[0], out.ctypes.data)
    return out


def _raw_ciphertexts(p, moduli, D, repr, seed):
    """raw (c1, c2) in `repr` and the reduced NTT-domain copies the oracle takes"""
    orc = O.Oracle(moduli, p.l)
    c1_raw, c1_red = unreduced(_uniform(moduli, (D, p.k, p.L, p.l), seed), moduli, seed + 1)
    c2_raw, c2_red = unreduced(_uniform(moduli, (D, p.n, p.L, p.l), seed + 2), moduli, seed + 3)
    if repr == P.REPR_POWER:
        c1_red, c2_red = orc.ntt_forward(c1_red), orc.ntt_forward(c2_red)
    return c1_raw, c2_raw, c1_red, c2_red


# (chain, n, k, l, D): k = 64 keeps decrypt_mac whole (c2 in its own pass), k = 256 with few dealers splits the terms
# (c2 in decrypt_finish); L l >= 256 takes the full-width form, smaller the dealer-grouped one
# (chain, n, k, l, D): ... and L l / 2 > 1024 (33 limbs at l = 64) the generic decrypt_mac_kernel
DECRYPT_CASES = [
    ("example56", 30, 64, 8, 7),
    ("bench61_fw", 24, 64, 16, 5),
    ("test40_split", 26, 256, 16, 3),
    ("top62", 24, 64, 8, 2),
    ("tiny_among_56", 24, 32, 8, 4),
    ("wide33_generic", 6, 8, 64, 2),
]


def _decrypt_chain(name):
    return {"bench61_fw": M.bench_moduli(17), "test40_split": TEST_MODULI,
            "wide33_generic": primes_1mod(128, 33)}.get(name) or CHAINS[name]


@pytest.mark.parametrize("repr", [P.REPR_NTT, P.REPR_POWER], ids=["ntt", "power"])
@pytest.mark.parametrize("chain,n,k,l,D", DECRYPT_CASES, ids=[c[0] for c in DECRYPT_CASES])
def test_raw_ciphertexts_into_every_decrypt(chain, n, k, l, D, repr):
    moduli = _decrypt_chain(chain)
    p = _params(n, k, l, moduli)
    orc = O.Oracle(moduli, l)
    c1_raw, c2_raw, c1_red, c2_red = _raw_ciphertexts(p, moduli, D, repr, seed=k + D + repr)
    rng = np.random.default_rng(D)
    sk = rng.integers(-1, 2, size=(n, k, l), dtype=np.int64)
    for i, v in enumerate(I64_EXTREMES + [moduli[-1], -moduli[-1]]):
        sk[i % 3, (5 * i) % k, (3 * i) % l] = v                        # parties 0..2: signed extremes
    for party in (0, 2, n - 1):
        noisy_o = orc.decrypt_noisy(sk[party], c1_red, c2_red[:, party])
        want = _decode_host(p, noisy_o)
        out, nz = _decrypt_batch(p, sk[party], c1_raw.copy(), c2_raw[:, party].copy(), repr)
        assert np.array_equal(nz, noisy_o) and _below_q(nz, moduli), f"noisy party {party}"
        assert np.array_equal(out, want), f"party {party}"
        # ... and the HIP path on the reduced words (POWER: the reduced power-basis words)
        red1, red2 = (c1_red, c2_red[:, party]) if repr == P.REPR_NTT else (orc.ntt_inverse(c1_red), orc.ntt_inverse(c2_red[:, party]))
        out_r, nz_r = _decrypt_batch(p, sk[party], red1, red2, repr)
        assert np.array_equal(out_r, out) and np.array_equal(nz_r, nz)
    # every party: both sides of the 22-party dispatch
    for lo, hi in ((0, n), (n - 4, n)):
        got = _decrypt_all(p, lo, hi, sk[lo:hi], c1_raw, c2_raw, repr)
        for i in sorted({0, 1, 2, hi - lo - 1} & set(range(hi - lo))):
            want = _decode_host(p, orc.decrypt_noisy(sk[lo + i], c1_red, c2_red[:, lo + i]))
            assert np.array_equal(got[i], want), f"decrypt_all [{lo}, {hi}) party {lo + i}"


def test_dealt_shares_from_raw_ciphertext_words():
    # real ciphertexts (keys and shares of 24 dealers for 40 parties) handed over as raw words w + t q, whole polynomials at
    # the largest t: every party on the matrix cores and on the per-party path must recover the dealt shares, and equal the
    # oracle on the reduced words (random residues mostly decode to 0, which would hide a wrong c2)
    n, k, l, moduli, D = 40, 16, 8, EXAMPLE_MODULI, 24
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    shares = [[(d * 7919 + j * 104729 + 1) % (1 << 32) for j in range(n)] for d in range(D)]
    cts = P.encrypt_many(shares, gpk, [P.api._dealer_seed(SEED, d) for d in range(D)])
    c1 = np.stack([ct.c1 for ct in cts])
    c2 = np.stack([ct.c2 for ct in cts])
    c1_raw, c1_red = unreduced(c1, moduli, 11, classes=False)
    c2_raw, c2_red = unreduced(c2, moduli, 12, classes=False)
    assert np.array_equal(c1_red, c1) and np.array_equal(c2_red, c2) and (c2_raw != c2).mean() > 0.7
    sk = np.stack([pt.secret_key.secret_coeffs for pt in parties])
    got = _decrypt_all(p, 0, n, sk, c1_raw, c2_raw, P.REPR_NTT)
    assert (got == np.array(shares, dtype=np.uint64).T).mean() >= 0.99
    orc = O.Oracle(moduli, l)
    for i in (0, 17, n - 1):
        want = _decode_host(p, orc.decrypt_noisy(sk[i], c1_red, c2_red[:, i]))
        assert np.array_equal(got[i], want), f"party {i}"
        out, _ = _decrypt_batch(p, sk[i], c1_raw, c2_raw[:, i], P.REPR_NTT)
        assert np.array_equal(out, want), f"per-party {i}"


# ------------------------------------------------------------------------------------------- transforms and decode
@pytest.mark.parametrize("chain,l", [("example56", 8), ("bench61", 32), ("test40", 16), ("top62", 64), ("tiny_among_56", 8)])
def test_raw_polynomials_through_the_transforms(chain, l):
    moduli = CHAINS[chain]
    p = _params(8, 4, l, moduli)
    orc = O.Oracle(moduli, l)
    for count in (40, 3000):                                   # small batches (LDS form) and large ones (per-thread form)
        raw, red = unreduced(_uniform(moduli, (count, len(moduli), l), count + l), moduli, l)
        fw, iv = p.ntt_forward(raw), p.ntt_inverse(raw)
        assert _below_q(fw, moduli) and _below_q(iv, moduli)
        assert np.array_equal(fw, orc.ntt_forward(red))
        assert np.array_equal(iv, orc.ntt_inverse(red))


@pytest.mark.parametrize("chain,l", [("example56", 8), ("bench61", 16), ("test40", 8), ("top62", 8), ("tiny_among_56", 8)])
def test_raw_noisy_residues_into_the_decode(chain, l):
    moduli = CHAINS[chain]
    p = _params(8, 4, l, moduli)
    m = M.Params(8, 4, l, moduli)
    rng = np.random.default_rng(l)
    D = m.delta
    ring = [[(-(int(rng.integers(0, 1 << 32)) * D ** j) + int(rng.integers(-50, 51))) % m.Q for j in range(l)] for _ in range(48)]
    red = np.array([[[c % q for c in poly] for q in moduli] for poly in ring], dtype=np.uint64)
    raw, red2 = unreduced(red, moduli, 3)
    want = np.array([M.decode_scalar_pvw(M.from_rns([[int(v) for v in row] for row in x], list(moduli)), m) for x in red2],
                    dtype=np.uint64)
    assert np.array_equal(_decode_host(p, red2), want)
    assert np.array_equal(_decode_host(p, raw), want)
    out = np.zeros(len(raw), dtype=np.uint64)
    p._call("pvw_decode", np.ascontiguousarray(raw).ctypes.data, len(raw), out.ctypes.data)
    assert np.array_equal(out, want)


# ------------------------------------------------------------------------------------------- signed inputs, scalars
@pytest.mark.parametrize("chain,n,k,l,dealers", [("bench61", 12, 256, 8, (1, 2, 3)), ("example56", 12, 64, 8, (1, 2, 4))])
def test_explicit_randomness_and_scalars_at_their_extremes(chain, n, k, l, dealers):
    # explicit r / e1 / e2 at INT64_MIN, INT64_MAX, +-q, +-2^62 (the compact addends of mac_small_make), scalars over the
    # whole u64 range (read as i64); multi-dealer scalars through the VALU and the GEMM finish with fused e2
    _extremes_case(chain, n, k, l, dealers)


@pytest.fixture
def tuning_library():
    """contexts created inside the test live in libpvw_hip_tuning.so (as in test_gpu_tuning.py)"""
    from pvw_rs_amd import _ffi
    prev = _ffi.select("tuning")
    yield
    _ffi.select(prev)


@pytest.mark.parametrize("chain,n,k,l,dealers", [("bench61", 12, 256, 8, (3,)), ("example56", 12, 64, 8, (4,))])
def test_scalars_through_the_gemm_finish_with_e2_from_the_prologue(chain, n, k, l, dealers, tuning_library, monkeypatch):
    # PVW_FUSED_E2=0 (tuning build): e2 + m g-hat come from the prologue as an addend of the c2 finish pass instead of
    # being drawn inside it -- the other GEMM finish form, with the same extreme scalars and explicit randomness
    monkeypatch.setenv("PVW_FUSED_E2", "0")
    _extremes_case(chain, n, k, l, dealers)


def _extremes_case(chain, n, k, l, dealers):
    moduli = CHAINS[chain]
    p = _params(n, k, l, moduli)
    orc = O.Oracle(moduli, l)
    crs = P.PvwCrs.new_deterministic(p, SEED)
    gpk = P.GlobalPublicKey.new(crs)
    gpk.fill_uniform(SEED)
    a_hat, b_hat = crs.matrix(P.REPR_NTT), gpk.matrix(repr=P.REPR_NTT)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    ext = I64_EXTREMES + [moduli[0], -moduli[0], moduli[-1] - 1]
    r, e1, e2 = _oracle_randomness(SEED, n, k, l)
    for i, v in enumerate(ext):
        r[i % k, i % l] = v
        e1[(3 * i) % k, (i + 1) % l] = v
        e2[i % n, (2 * i) % l] = v
    scalars = np.array([MAXW, 1 << 63, (1 << 63) - 1, 0, 1, (1 << 64) - 1000, 1 << 32] + list(range(n - 7)), dtype=np.uint64)
    ct = P.encrypt(scalars, gpk, r=r, e1=e1, e2=e2)
    c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, scalars, r, e1, e2)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    ct = P.encrypt(scalars, gpk, SEED)
    c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, scalars, *_oracle_randomness(SEED, n, k, l))
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    for D in dealers:
        rows = [list(np.roll(scalars, d)) for d in range(D)]
        seeds = [P.api._dealer_seed(SEED, d) for d in range(D)]
        many = P.encrypt_many(rows, gpk, seeds)
        for d in range(D):
            c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(rows[d], dtype=np.uint64), *_oracle_randomness(seeds[d], n, k, l))
            assert np.array_equal(many[d].c1, c1o) and np.array_equal(many[d].c2, c2o), f"D={D} dealer {d}"


def test_device_pointer_entry_points():
    # pvw_load_crs_device / pvw_load_pk_device on raw words; pvw_decrypt_batch_device, pvw_sk_load (sk at the signed
    # extremes) + pvw_decrypt_batch_device_sk, pvw_decrypt_all_device on both sides of the dispatch, pvw_decode_device
    _in_fresh_process("_device_body", 300)


# ------------------------------------------------------------------------------------------- device pointers
def _device_body():
    from test_gpu_decrypt_all import _Hip
    n, k, l, moduli = 30, 64, 8, EXAMPLE_MODULI
    L = len(moduli)
    p = _params(n, k, l, moduli)
    orc = O.Oracle(moduli, l)
    hip = _Hip()
    stream = hip.stream()
    bufs = []

    def up(a):
        bufs.append(hip.upload(a))
        return bufs[-1]

    try:
        # public key and CRS from device pointers (raw NTT-domain words), then encrypt against the oracle
        a_raw, a_red = unreduced(_uniform(moduli, (k, k, L, l), 1), moduli, 2)
        b_raw, b_red = unreduced(_uniform(moduli, (n, k, L, l), 3), moduli, 4)
        p._call("pvw_load_crs_device", up(a_raw), P.REPR_NTT, stream)
        gpk = P.GlobalPublicKey.new(P.PvwCrs(p))
        p._call("pvw_load_pk_device", 0, n, up(b_raw), P.REPR_POWER, stream)
        hip.sync(stream)
        b_hat = orc.ntt_forward(b_red)
        scalars = np.arange(n, dtype=np.uint64)
        ct = P.encrypt(scalars, gpk, SEED)
        c1o, c2o = orc.encrypt(a_red, b_hat, p.gadget_polynomial(P.REPR_NTT), scalars, *_oracle_randomness(SEED, n, k, l))
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
        # ciphertexts from device pointers: decrypt_batch_device, _device_sk, decrypt_all_device, decode_device
        D = 6
        c1_raw, c2_raw, c1_red, c2_red = _raw_ciphertexts(p, moduli, D, P.REPR_NTT, seed=5)
        sk = np.random.default_rng(2).integers(-1, 2, size=(n, k, l), dtype=np.int64)
        for i, v in enumerate(I64_EXTREMES + [moduli[1], -moduli[1]]):
            sk[0, (7 * i) % k, i % l] = v
        party = 0
        noisy_o = orc.decrypt_noisy(sk[party], c1_red, c2_red[:, party])
        want = _decode_host(p, noisy_o)
        d_c1, d_c2col, d_sk = up(c1_raw), up(np.ascontiguousarray(c2_raw[:, party])), up(sk[party])
        d_nz, d_out = up(np.zeros((D, L, l), dtype=np.uint64)), up(np.zeros(D, dtype=np.uint64))
        p._call("pvw_decrypt_batch_device", d_sk, d_c1, d_c2col, D, P.REPR_NTT, d_nz, d_out, stream)
        hip.sync(stream)
        assert np.array_equal(hip.download(d_out, (D,)), want)
        dk = C.c_void_p()
        skc = np.ascontiguousarray(sk[party])
        p._call("pvw_sk_load", skc.ctypes.data, C.byref(dk))
        try:
            p._call("pvw_decrypt_batch_device_sk", dk, d_c1, d_c2col, D, P.REPR_NTT, d_nz, d_out, stream)
            hip.sync(stream)
            assert np.array_equal(hip.download(d_out, (D,)), want)
        finally:
            P.api._check(p._lib.pvw_sk_free(dk))
        d_all_out = up(np.zeros((n, D), dtype=np.uint64))
        d_c2, d_skall = up(c2_raw), up(sk)
        for lo, hi in ((0, n), (0, 3)):
            p._call("pvw_decrypt_all_device", lo, hi, d_skall, d_c1, d_c2, D, P.REPR_NTT, d_all_out, stream)
            hip.sync(stream)
            got = hip.download(d_all_out, (hi - lo, D))
            for i in (0, hi - lo - 1):
                assert np.array_equal(got[i], _decode_host(p, orc.decrypt_noisy(sk[lo + i], c1_red, c2_red[:, lo + i]))), (lo, hi, i)
        raw_nz, red_nz = unreduced(noisy_o, moduli, 6)
        p._call("pvw_decode_device", up(raw_nz), D, d_out, stream)
        hip.sync(stream)
        assert np.array_equal(hip.download(d_out, (D,)), _decode_host(p, red_nz))
    finally:
        hip.sync()
        for b in bufs:
            hip.free(b)
        hip.L.hipStreamDestroy(stream)


def _in_fresh_process(body, timeout):
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = {[here, os.path.dirname(here), os.path.join(os.path.dirname(here), 'oracle')]!r}; " \
           f"import test_gpu_unreduced_words as t; t.{body}(); print('BODY_OK')"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "BODY_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

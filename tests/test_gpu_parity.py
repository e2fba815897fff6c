"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI,
against the oracle (big-integer model + C restatement) and the committed golden fixtures.
All comparisons are bit-exact (integer arithmetic)."""
import glob
import os

import numpy as np
import pytest

import pvw_model as M
import pvw_oracle as O
import pvw_rs_amd as P
from _util import EXAMPLE_MODULI, SEED, TEST_MODULI, decode_cases, make_system, primes_1mod, rns_to_ring

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))


def build_params(n, k, l, moduli, variance=0.5, bounds=(100, 200), shard=None):
    b = (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
         .set_secret_variance(variance).set_error_bounds(*bounds))
    if shard:
        b.set_shard(*shard)
    return b.build()


def params_from_golden(z, shard=None):
    return build_params(int(z["n"]), int(z["k"]), int(z["l"]), [int(q) for q in z["moduli"]],
                        float(z["variance"]), (int(z["bound1"]), int(z["bound2"])), shard)


def test_device_is_gfx950():
    assert P.device_available(), "these tests need the HIP path; there is no CPU fallback"


# ---------------------------------------------------------------- ring primitives
@pytest.mark.parametrize("l", [8, 16, 32, 64])
@pytest.mark.parametrize("moduli", [TEST_MODULI, M.bench_moduli(17)], ids=["test3", "bench17"])
def test_ntt_round_trip_and_oracle(l, moduli):
    if l == 64 and len(moduli) == 17:
        moduli = primes_1mod(128, 17)          # the bench chain is only 1 mod 64
    p = build_params(3, 4, l, moduli)
    orc = O.Oracle(moduli, l)
    rng = np.random.default_rng(l)
    polys = np.stack([rng.integers(0, q, size=(37, l), dtype=np.uint64) for q in moduli], axis=1)
    fwd = p.ntt_forward(polys)
    assert np.array_equal(fwd, orc.ntt_forward(polys))
    assert np.array_equal(p.ntt_inverse(fwd), polys)
    small = rng.integers(-(1 << 62), 1 << 62, size=(11, l), dtype=np.int64)
    small[0, :4] = [0, -1, np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    assert np.array_equal(p.from_coefficients(small, P.REPR_NTT), orc.small_to_ntt(small))
    want_pb = np.array([[[int(c) % q for c in row] for q in moduli] for row in small], dtype=np.uint64)
    assert np.array_equal(p.from_coefficients(small, P.REPR_POWER), want_pb)


def test_encode_scalar_matches_model():
    # parameters.rs:346-367 incl. negative scalars
    p = build_params(3, 4, 8, TEST_MODULI)
    m = M.Params(3, 4, 8, TEST_MODULI)
    for s in (0, 1, 42, -7, (1 << 63) - 1, -(1 << 63)):
        enc = p.encode_scalar(s, P.REPR_POWER)
        assert p.poly_to_bigints(enc) == m.encode_scalar(s)
        assert np.array_equal(p.ntt_inverse(p.encode_scalar(s, P.REPR_NTT)[None])[0], enc)


# ---------------------------------------------------------------- samplers
def test_samplers_match_oracle_and_statistics():
    p = build_params(3, 4, 16, TEST_MODULI)
    for var in (0.5, 1.0, 2.0, 3.0, 10.0, 16.0):
        got = p.sample_vec_cbd(SEED, P.DOM_R, 9, 300, var)
        assert np.array_equal(got, O.sample_cbd(SEED, M.DOM_R, 9, 300, 16, var))
    xs = p.sample_vec_cbd(SEED, P.DOM_SK, 0, 1000, 0.5).reshape(-1)       # tests/sampling.rs:198-274
    assert set(np.unique(xs)) <= {-1, 0, 1} and abs(xs.mean()) < 0.1 and abs(xs.var() - 0.5) < 0.1
    for bound in (1, 50, 200, 1172385, (1 << 31) - 1, 1 << 32, (1 << 40) + 12345, 1 << 61):
        got = p.sample_uniform_coefficients(SEED, P.DOM_E2, 3, 200, bound)
        assert np.array_equal(got, O.sample_uniform(SEED, M.DOM_E2, 3, 200, 16, bound))
        assert got.min() >= -bound and got.max() <= bound
    for bad in (0.3, 0.7, 17.0):
        with pytest.raises(P.PvwError) as e:
            p.sample_vec_cbd(SEED, P.DOM_R, 0, 1, bad)
        assert e.value.variant == "SamplingError"


def test_gaussian_contract():
    # normal.rs:136-162; tests/sampling.rs:15-195 (bounds respected, sign mix, scale ordering)
    p = build_params(3, 4, 8, TEST_MODULI)
    assert np.all(p.sample_discrete_gaussian_vec(SEED, 0, 64) == 0)
    for bound in (1, 4, 100, 10 ** 6, 10 ** 12):
        xs = p.sample_discrete_gaussian_vec(SEED, bound, 4096)
        assert xs.min() >= -bound and xs.max() <= bound
        if bound >= 100:
            assert (xs > 0).any() and (xs < 0).any()
    small = np.abs(p.sample_discrete_gaussian_vec(SEED, 4, 4096)).mean()
    large = np.abs(p.sample_discrete_gaussian_vec(SEED, 10 ** 6, 4096)).mean()
    assert large > small
    # bound <= 5: sigma = bound/16.96 <= 0.3 -> genuinely Gaussian ratio, almost always rounds to 0 or +-1
    xs = p.sample_discrete_gaussian_vec(SEED, 4, 4096)
    assert np.abs(xs).max() <= 4 and (xs == 0).mean() > 0.3
    # the model's stream gives the same integers for the uniform branches (no libm involved)
    rng_vals = []
    for i in range(32):
        rng_vals.append(M.sample_single_gaussian(10 ** 6, M.ChaChaRng(SEED, M.DOM_GAUSS, i)))
    assert p.sample_discrete_gaussian_vec(SEED, 10 ** 6, 32).tolist() == rng_vals
    huge = p.sample_discrete_gaussian_vec(SEED, 10 ** 16, 256)
    assert np.abs(huge).max() <= 10 ** 6
    assert huge.tolist() == [M.sample_single_gaussian(10 ** 16, M.ChaChaRng(SEED, M.DOM_GAUSS, i)) for i in range(256)]


def test_gaussian_box_muller_branch_moments_and_model_draws():
    # normal.rs:165-190: for bound <= 5, sigma = bound/16.96 <= 0.3 and the ratio is a genuine Box-Muller draw
    # z*sigma, rejected outside [-1, 1]; x = round(ratio*bound) = round(z * bound^2/16.96).  The reference's
    # own moment check (tests/sampling.rs:114-129) asks |mean| < 0.2 and |var - 1| < 0.3 of N(0,1) on 1000 draws;
    # here the expected moments of the ROUNDED variable are computed from the normal CDF and held to the same
    # relative slack on 8192 draws per bound, and every draw is compared with the model's draw on the same
    # ChaCha stream: libm's and the device's log / cos may differ in the last ulp, which can only matter when
    # z*scale sits within ~1e-15 of a rounding boundary or of the rejection edge -- counted, and bounded.
    import math
    p = build_params(3, 4, 8, TEST_MODULI)
    N = 8192
    phi = lambda t: 0.5 * (1.0 + math.erf(t / math.sqrt(2.0)))
    total_mismatch = 0
    for bound in (1, 2, 3, 4, 5):
        xs = p.sample_discrete_gaussian_vec(SEED, bound, N)
        assert np.abs(xs).max() <= bound
        scale = bound * bound / 16.96                       # x = round(z * scale), z truncated to |z| <= 16.96/bound
        zmax = 16.96 / bound
        norm = phi(zmax) - phi(-zmax)
        probs = {}
        for j in range(-bound, bound + 1):
            lo, hi = max((j - 0.5) / scale, -zmax), min((j + 0.5) / scale, zmax)
            probs[j] = max(phi(hi) - phi(lo), 0.0) / norm
        var_want = sum(j * j * q for j, q in probs.items())
        sd = math.sqrt(var_want) if var_want > 0 else 0.0
        assert abs(xs.mean()) < 0.2 * max(sd, 0.05), (bound, xs.mean())
        assert abs(xs.var() - var_want) < 0.3 * max(var_want, 0.01), (bound, xs.var(), var_want)
        for j, q in probs.items():                           # the whole histogram, not only two moments
            assert abs((xs == j).mean() - q) < 5.0 * math.sqrt(max(q * (1 - q), 1e-6) / N) + 1e-3, (bound, j)
        want = [M.sample_single_gaussian(bound, M.ChaChaRng(SEED, M.DOM_GAUSS, i)) for i in range(N)]
        total_mismatch += int((xs != np.array(want)).sum())
    assert total_mismatch <= 2, f"{total_mismatch} of {5 * N} Box-Muller draws differ from the model"


# ---------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(g)[:-4] for g in GOLDEN])
def test_golden_keygen_encrypt_decrypt(path):
    z = np.load(path)
    p = params_from_golden(z)
    n, k = p.n, p.k
    assert p.roots() == [int(x) for x in z["psi"]]
    crs = P.PvwCrs.from_polynomials(p, z["A_pb"], P.REPR_POWER)
    assert np.array_equal(crs.matrix(P.REPR_POWER), z["A_pb"])
    gpk = P.GlobalPublicKey.new(crs)
    assert not gpk.is_full() and gpk.num_public_keys() == 0
    # keygen on the device with the fixture's secrets and key errors
    gpk.generate_with_errors(0, z["sk"], z["ek"])
    assert gpk.is_full() and gpk.num_public_keys() == n
    assert np.array_equal(gpk.matrix(repr=P.REPR_POWER), z["B_pb"])
    # encrypt with the fixture's randomness, both output representations
    ct = P.encrypt(z["scalars"], gpk, r=z["r"], e1=z["e1"], e2=z["e2"], repr=P.REPR_POWER)
    assert np.array_equal(ct.c1, z["c1_pb"]) and np.array_equal(ct.c2, z["c2_pb"])
    ct_ntt = P.encrypt(z["scalars"], gpk, r=z["r"], e1=z["e1"], e2=z["e2"], repr=P.REPR_NTT)
    assert np.array_equal(p.ntt_inverse(ct_ntt.c1), z["c1_pb"])
    assert np.array_equal(p.ntt_inverse(ct_ntt.c2), z["c2_pb"])
    # decrypt every party, from both representations
    for ctx in (ct, ct_ntt):
        for i in range(n):
            sk = P.SecretKey.from_coefficients(p, z["sk"][i])
            vals, noisy = P.api._decrypt_batch(p, [ctx], sk, i, return_noisy=True)
            assert np.array_equal(noisy[0], z["noisy_pb"][i])
            assert vals[0] == int(z["decoded"][i])


@pytest.mark.parametrize("path", GOLDEN[:2], ids=[os.path.basename(g)[:-4] for g in GOLDEN[:2]])
def test_golden_load_pk_paths(path):
    # add_public_key one party at a time, in NTT form computed by the oracle, then encrypt
    z = np.load(path)
    p = params_from_golden(z)
    moduli = [int(q) for q in z["moduli"]]
    orc = O.Oracle(moduli, p.l)
    crs = P.PvwCrs.from_polynomials(p, orc.ntt_forward(z["A_pb"]), P.REPR_NTT)
    gpk = P.GlobalPublicKey.new(crs)
    b_hat = orc.ntt_forward(z["B_pb"])
    for i in reversed(range(p.n)):
        gpk.add_public_key(i, b_hat[i], P.REPR_NTT)
        assert gpk.num_public_keys() == p.n                      # public_key.rs:245: max index + 1
    assert np.array_equal(gpk.get_polynomial(1, 2, P.REPR_POWER), z["B_pb"][1, 2])
    assert gpk.get_polynomial(p.n, 0) is None
    ct = P.encrypt(z["scalars"], gpk, r=z["r"], e1=z["e1"], e2=z["e2"], repr=P.REPR_NTT)
    g_hat = orc.ntt_forward(z["g_pb"][None])[0]
    c1o, c2o = orc.encrypt(orc.ntt_forward(z["A_pb"]), b_hat, g_hat, z["scalars"], z["r"], z["e1"], z["e2"])
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)   # NTT domain, same psi rule


# ---------------------------------------------------------------- reference-shaped end-to-end tests
def setup_system(n, k, l, moduli, variance=0.5, seed=SEED):
    b1, b2 = P.PvwParameters.suggest_error_bounds(n, k, l, moduli, variance)
    p = build_params(n, k, l, moduli, variance, (b1, b2))
    parties = [P.Party.new(i, p, seed) for i in range(n)]
    crs = P.PvwCrs.new_deterministic(p, seed)
    gpk = P.GlobalPublicKey.new(crs)
    gpk.generate_all_party_keys(parties, seed)
    return p, gpk, parties


def test_basic_encryption_shapes_and_wrappers():
    # tests/crypto.rs:91-149
    p, gpk, _ = setup_system(3, 4, 8, TEST_MODULI)
    ct = P.encrypt([10, 20, 30], gpk, SEED)
    ct.validate()
    assert len(ct) == p.n and len(ct.c1) == p.k and len(ct.c2) == p.n
    assert ct.get_party_ciphertext(p.n) is None and ct.get_party_ciphertext(0) is not None
    assert len(P.encrypt_party_shares([10000, 20000, 30000], 1, gpk, SEED)) == 3
    cts = P.encrypt_all_party_shares([[11, 12, 13], [21, 22, 23], [31, 32, 33]], gpk, SEED)
    assert len(cts) == 3 and all(len(c) == 3 for c in cts)
    assert not np.array_equal(cts[0].c1, cts[1].c1)            # every dealer has its own randomness
    assert len(P.encrypt_broadcast(999, gpk, SEED)) == 3
    # determinism: same seed, same ciphertext
    assert np.array_equal(P.encrypt([10, 20, 30], gpk, SEED).c2, ct.c2)


def test_invalid_inputs():
    # tests/crypto.rs:181-207
    p, gpk, _ = setup_system(3, 4, 8, TEST_MODULI)
    for bad in ([1, 2], [1, 2, 3, 4]):
        with pytest.raises(P.PvwError) as e:
            P.encrypt(bad, gpk, SEED)
        assert e.value.variant == "InvalidParameters" and "Must provide exactly n=3 scalars" in str(e.value)
    with pytest.raises(P.PvwError):
        P.encrypt_party_shares([1, 2, 3], 999, gpk, SEED)
    with pytest.raises(P.PvwError):
        P.encrypt_all_party_shares([[1, 2], [3, 4, 5], [6, 7, 8]], gpk, SEED)
    with pytest.raises(P.PvwError):
        P.Party.new(3, p, SEED)                                   # tests/keys.rs:53-64
    # incomplete global key (encryption.rs:117-121)
    p2 = build_params(3, 4, 8, TEST_MODULI)
    crs = P.PvwCrs.new_deterministic(p2, SEED)
    gpk2 = P.GlobalPublicKey.new(crs)
    gpk2.generate_and_add_party(P.Party.new(0, p2, SEED), SEED)
    with pytest.raises(P.PvwError) as e:
        P.encrypt([1, 2, 3], gpk2, SEED)
    assert "not complete" in str(e.value)
    # failing correctness gate (encryption.rs:124-128)
    p3 = build_params(3, 4, 8, [0xFFFFEE001], 0.5, (1 << 50, 1 << 50))
    gpk3 = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p3, SEED))
    gpk3.fill_uniform(SEED)
    with pytest.raises(P.PvwError) as e:
        P.encrypt([1, 2, 3], gpk3, SEED)
    assert "correctness condition" in str(e.value)
    with pytest.raises(P.PvwError):
        P.decrypt_party_shares([], P.SecretKey.random(p, SEED, 0), 0)


@pytest.mark.parametrize("n,k,l,moduli,variance", [
    (10, 4, 16, TEST_MODULI, 0.5),        # tests/crypto.rs:237-305 test_decryption_l16
    (7, 32, 8, TEST_MODULI, 0.5),         # examples/pvw_valid_dec.rs commented config
    (5, 64, 8, EXAMPLE_MODULI, 10.0),     # examples/pvw_valid_dec.rs:40-52 at reduced k
])
def test_decryption_round_trip(n, k, l, moduli, variance):
    if variance == 10.0:
        p = build_params(n, k, l, moduli, variance, (1, 1172385))
        parties = [P.Party.new(i, p, SEED) for i in range(n)]
        gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
        gpk.generate_all_party_keys(parties, SEED)
    else:
        p, gpk, parties = setup_system(n, k, l, moduli, variance)
    all_vectors = [[dealer * 100 + j for j in range(1, n + 1)] for dealer in range(n)]
    cts = P.encrypt_all_party_shares(all_vectors, gpk, SEED)
    correct = total = 0
    for idx, party in enumerate(parties):
        shares = P.decrypt_party_shares(cts, party.secret_key, idx)
        for dealer, v in enumerate(shares):
            correct += v == all_vectors[dealer][idx]
            total += 1
        assert P.decrypt_party_value(cts[0], party.secret_key, idx) == shares[0]
    assert correct / total >= 0.95


def test_seed_mode_equals_explicit_mode_with_oracle_samples():
    n, k, l, moduli = 12, 8, 16, M.bench_moduli(5)
    p = build_params(n, k, l, moduli, 3.0, (77, 1 << 33))
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    scalars = [(i * 1000 + 1) % (1 << 32) for i in range(n)]
    ct = P.encrypt(scalars, gpk, SEED)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 3.0)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 77)
    e2 = O.sample_uniform(SEED, M.DOM_E2, 0, n, l, 1 << 33)
    ct2 = P.encrypt(scalars, gpk, r=r, e1=e1, e2=e2)
    assert np.array_equal(ct.c1, ct2.c1) and np.array_equal(ct.c2, ct2.c2)
    # and both equal the C oracle on the same synthetic A-hat / B-hat
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, len(moduli), l)
    b_hat = orc.fill_uniform(SEED, M.DOM_PK, 0, n * k).reshape(n, k, len(moduli), l)
    assert np.array_equal(gpk.crs.matrix(P.REPR_NTT), a_hat)
    assert np.array_equal(gpk.matrix(repr=P.REPR_NTT), b_hat)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(scalars, dtype=np.uint64), r, e1, e2)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)


@pytest.mark.parametrize("n,k,l,L", [
    (33, 7, 8, 3),        # ragged: k not a multiple of 4, n not a multiple of the tile rows
    (5, 1, 8, 2),         # k = 1 (tests/params.rs:253)
    (19, 130, 16, 4),     # k > one staged chunk per wave
    (9, 300, 32, 2),      # l = 32, several r-hat chunks
    (6, 24, 64, 2),       # l = 64
    (1, 5, 8, 1),         # single party, single limb
])
def test_ragged_geometries_against_c_oracle(n, k, l, L):
    moduli = M.bench_moduli(L) if l <= 32 else primes_1mod(128, L)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    scalars = [(i * 1000 + 1) % (1 << 32) for i in range(n)]
    ct = P.encrypt(scalars, gpk, SEED)
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, L, l)
    b_hat = orc.fill_uniform(SEED, M.DOM_PK, 0, n * k).reshape(n, k, L, l)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(SEED, M.DOM_E2, 0, n, l, 200)
    c1o, c2o = orc.encrypt(a_hat, b_hat, p.gadget_polynomial(P.REPR_NTT), np.array(scalars, dtype=np.uint64), r, e1, e2)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    # batched decrypt of D copies against the C oracle (noisy polynomials, power basis)
    sk = O.sample_cbd(SEED, M.DOM_SK, 0, k, l, 0.5)
    D = 5
    c1s = np.stack([np.roll(ct.c1, d, axis=0) for d in range(D)])
    c2col = np.stack([ct.c2[d % n] for d in range(D)])
    cts = [P.PvwCiphertext(c1s[d], np.repeat(c2col[d][None], n, axis=0), p, P.REPR_NTT) for d in range(D)]
    vals, noisy = P.api._decrypt_batch(p, cts, P.SecretKey.from_coefficients(p, sk), 0, return_noisy=True)
    assert np.array_equal(noisy, orc.decrypt_noisy(sk, c1s, c2col))


MAC_SCHEDULE_CASES = [(40, 256, 8, 3), (21, 128, 16, 2), (9, 64, 8, 2), (5, 24, 8, 2)]
# geometries that qualify for the 61-bit packed stream (l <= 16, k a multiple of 256): one and two periods per wave,
# ragged row blocks, l = 8 and 16, three periods (k = 768)
MAC_PACKED_CASES = [(40, 256, 8, 3), (19, 512, 16, 2), (133, 512, 8, 2), (9, 768, 8, 2), (70, 256, 16, 3)]
# narrower modulus chains stream at 40 / 48 / 56 bits per residue (k a multiple of 64): the reference's own sets --
# 36/37-bit (tests/crypto.rs:52) and 56-bit (examples/pvw_valid_dec.rs:40-45) -- and a 48-bit chain; one to five groups
# of 16 j per wave (k = 64 .. 320), ragged row blocks, l = 8 and 16
MAC_PACKED_WIDTH_CASES = [
    (40, 256, 8, TEST_MODULI, 40), (9, 64, 8, TEST_MODULI, 40), (21, 128, 16, TEST_MODULI, 40), (33, 320, 8, TEST_MODULI, 40),
    (40, 256, 8, primes_1mod(64, 3, top=1 << 48), 48), (17, 192, 16, primes_1mod(64, 2, top=1 << 48), 48),
    (40, 256, 8, EXAMPLE_MODULI, 56), (11, 64, 16, EXAMPLE_MODULI, 56), (5, 1024, 8, EXAMPLE_MODULI, 56),
    (23, 576, 8, EXAMPLE_MODULI[:2], 56),
]


def mac_rows_case(n, k, l, L, moduli=None):
    """(encrypt closure, oracle c1, oracle c2) for one geometry: c1, c2 of encryption.rs:158,177-200"""
    moduli = moduli or M.bench_moduli(L)
    L = len(moduli)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    scalars = [(i * 77 + 5) % (1 << 32) for i in range(n)]
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, L, l)
    b_hat = orc.fill_uniform(SEED, M.DOM_PK, 0, n * k).reshape(n, k, L, l)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(SEED, M.DOM_E2, 0, n, l, 200)
    c1o, c2o = orc.encrypt(a_hat, b_hat, p.gadget_polynomial(P.REPR_NTT), np.array(scalars, dtype=np.uint64), r, e1, e2)
    run = lambda: P.encrypt(scalars, gpk, SEED)   # noqa: E731
    run.params = p
    return run, c1o, c2o


@pytest.mark.parametrize("n,k,l,L", MAC_SCHEDULE_CASES)
def test_mac_rows_shape_selected_schedule_agrees_with_c_oracle(n, k, l, L):
    # the schedule the shipped library picks by shape (every other one: tests/test_gpu_tuning.py)
    run, c1o, c2o = mac_rows_case(n, k, l, L)
    ct = run()
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)


@pytest.mark.parametrize("n,k,l,L", MAC_PACKED_CASES)
def test_mac_rows_over_the_packed_matrix_agrees_with_c_oracle(n, k, l, L):
    # mac_rows_packed_kernel: the tiled matrix is streamed from a 61-bit-per-residue copy (pack61_kernel); twice, so
    # that the second call reuses the copy, then after the public key has changed (the copy must be rebuilt)
    run, c1o, c2o = mac_rows_case(n, k, l, L)
    for _ in range(2):
        ct = run()
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
        assert run.params.packed_active() == 61               # the packed kernel is what ran, not a silent fall-back


@pytest.mark.parametrize("n,k,l,moduli,width", MAC_PACKED_WIDTH_CASES)
def test_mac_rows_streams_at_the_modulus_width(n, k, l, moduli, width):
    # mac_rows_packedw_kernel: residues of a 36/37-, 48- or 56-bit chain stored at 40 / 48 / 56 bits (pack_kernel)
    run, c1o, c2o = mac_rows_case(n, k, l, None, moduli)
    for _ in range(2):
        ct = run()
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
        assert run.params.packed_active() == width


def test_prepare_builds_the_derived_copies_up_front():
    # pvw_prepare: allocation, build and synchronisation happen there; a key change invalidates the copies of the
    # matrix it touched and a second prepare rebuilds them in place (no new allocation)
    n, k, l = 40, 256, 8
    moduli = M.bench_moduli(2)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    assert p.packed_active() == 0 and p.derived_bytes() == (0, 0)
    taken = p.prepare(P.PREPARE_PACKED | P.PREPARE_MFMA)
    packed_b, mfma_b = p.derived_bytes()
    crs_b, pk_b = p.resident_bytes()
    assert p.packed_active() == 61 and taken == packed_b + mfma_b
    assert packed_b == (crs_b + pk_b) * 61 // 64 and mfma_b >= crs_b + pk_b
    assert p.prepare(P.PREPARE_PACKED | P.PREPARE_MFMA) == 0            # nothing left to build
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, 2, l)
    scalars = np.arange(1, n + 1, dtype=np.uint64)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(SEED, M.DOM_E2, 0, n, l, 200)
    for seed in (SEED, bytes([0x31]) * 32):
        gpk.fill_uniform(seed)                                           # B-hat changed: its packed copy is stale
        assert p.packed_active() == 0
        assert p.prepare(P.PREPARE_PACKED) == 0 and p.packed_active() == 61 and p.derived_bytes()[0] == packed_b
        b_hat = orc.fill_uniform(seed, M.DOM_PK, 0, n * k).reshape(n, k, 2, l)
        c1o, c2o = orc.encrypt(a_hat, b_hat, p.gadget_polynomial(P.REPR_NTT), scalars, r, e1, e2)
        ct = P.encrypt(scalars, gpk, SEED)
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)


def test_encrypt_into_pinned_host_buffers():
    # pvw_host_alloc: output buffers the device can write -- pvw_encrypt then has the MAC store c1 / c2 straight into them
    # (NTT output; power-basis output and pageable buffers take the copy): same ciphertexts either way
    import ctypes as C
    from pvw_rs_amd import _ffi
    run, c1o, c2o = mac_rows_case(150, 256, 8, 3)
    p = run.params
    lib, n, k, L, l = p._lib, 150, 256, 3, 8
    bufs = []

    def pinned(shape):
        pp = C.c_void_p()
        assert lib.pvw_host_alloc(int(np.prod(shape)) * 8, C.byref(pp)) == 0
        bufs.append(pp)
        return np.ctypeslib.as_array((C.c_uint64 * int(np.prod(shape))).from_address(pp.value)).reshape(shape)

    c1p, c2p = pinned((k, L, l)), pinned((n, L, l))
    scal = np.array([(i * 77 + 5) % (1 << 32) for i in range(n)], dtype=np.uint64)
    rnd = _ffi.pvw_randomness_t()
    rnd.mode = _ffi.RND_SEED
    C.memmove(rnd.seed, SEED, 32)
    for repr_, want in ((P.REPR_NTT, (c1o, c2o)), (P.REPR_POWER, None)):
        c1p[:] = 0
        c2p[:] = 0
        rc = lib.pvw_encrypt(p._h, scal.ctypes.data_as(C.c_void_p), n, C.byref(rnd), c1p.ctypes.data_as(C.c_void_p),
                             c2p.ctypes.data_as(C.c_void_p), repr_)
        assert rc == 0, _ffi.last_error(lib)
        if want is None:
            want = (p.ntt_forward(c1p.copy()), p.ntt_forward(c2p.copy()))
            assert np.array_equal(want[0], c1o) and np.array_equal(want[1], c2o)
        else:
            assert np.array_equal(c1p, want[0]) and np.array_equal(c2p, want[1])
    del c1p, c2p
    for pp in bufs:
        assert lib.pvw_host_free(pp) == 0


def test_packed_matrix_follows_key_changes_and_wide_moduli_fall_back():
    n, k, l = 24, 256, 8
    moduli = M.bench_moduli(2)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, 2, l)
    scalars = np.arange(1, n + 1, dtype=np.uint64)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(SEED, M.DOM_E2, 0, n, l, 200)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    for seed in (SEED, bytes([0x77]) * 32, SEED):           # every refill invalidates the packed copy
        gpk.fill_uniform(seed)
        b_hat = orc.fill_uniform(seed, M.DOM_PK, 0, n * k).reshape(n, k, 2, l)
        c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, scalars, r, e1, e2)
        ct = P.encrypt(scalars, gpk, SEED)
        assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o) and p.packed_active() == 61
    # residues loaded UNREDUCED (r + q needs 62 bits): the copy would truncate them, so it must not be used
    b_hat = orc.fill_uniform(SEED, M.DOM_PK, 0, n * k).reshape(n, k, 2, l)
    unreduced = b_hat.copy()
    unreduced[3, 5] += np.array(moduli, dtype=np.uint64)[:, None]
    unreduced[n - 1, k - 1, 1, l - 1] += np.uint64(moduli[1])
    assert (unreduced >> np.uint64(61)).any()
    gpk.load_rows(0, unreduced, P.REPR_NTT)
    c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, scalars, r, e1, e2)
    ct = P.encrypt(scalars, gpk, SEED)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    assert p.packed_active() == 0                                      # the tiled matrices were streamed
    gpk.load_rows(0, b_hat, P.REPR_NTT)                                # reduced again: the packed stream comes back
    ct = P.encrypt(scalars, gpk, SEED)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o) and p.packed_active() == 61
    # a modulus of 62 bits does not fit the 61-bit stream: the unpacked kernel must serve it
    wide = primes_1mod(64, 2, top=(1 << 62) - 64)        # top must be a multiple of the step
    assert all(q >> 61 for q in wide)
    p2 = build_params(n, k, l, wide)
    gpk2 = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p2, SEED))
    gpk2.fill_uniform(SEED)
    orc2 = O.Oracle(wide, l)
    a2 = orc2.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, 2, l)
    b2 = orc2.fill_uniform(SEED, M.DOM_PK, 0, n * k).reshape(n, k, 2, l)
    c1o, c2o = orc2.encrypt(a2, b2, p2.gadget_polynomial(P.REPR_NTT), scalars, r, e1, e2)
    ct = P.encrypt(scalars, gpk2, SEED)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o) and p2.packed_active() == 0


DECRYPT_SHAPE_CASES = [
    (37, 16, 34, 5),      # 272 slot pairs (configs 4/5): four full waves + a 16-pair remainder wave
    (20, 32, 9, 4),       # 144 pairs: two full waves + remainder
    (64, 8, 17, 7),       # 68 pairs (configs 2/3): one full wave + a 4-pair remainder
    (9, 8, 3, 3),         # 12 pairs: remainder waves only
    (11, 16, 8, 2),       # 64 pairs: no remainder
    (300, 16, 34, 5),     # 272 pairs, k = 300: the inner products are cut into four ragged ranges of j (75 terms)
    (256, 8, 17, 6),      # 68 pairs (dealer-grouped form), four ranges of 64
    (512, 16, 4, 3),      # eight ranges of 64
]


def decrypt_mac_case(k, l, L, D, moduli=None):
    """(closure returning the noisy polynomials, oracle's) for decrypt_party_value's <sk, c1> - c2 (decryption.rs:257-274)"""
    moduli = moduli or M.bench_moduli(L)
    L = len(moduli)
    p = build_params(3, k, l, moduli)
    orc = O.Oracle(moduli, l)
    c1s = orc.fill_uniform(SEED, M.DOM_CRS, 0, D * k).reshape(D, k, L, l)
    c2col = orc.fill_uniform(SEED, M.DOM_PK, 0, D).reshape(D, L, l)
    sk = O.sample_cbd(SEED, M.DOM_SK, 0, k, l, 0.5)
    want = orc.decrypt_noisy(sk, c1s, c2col)
    cts = [P.PvwCiphertext(c1s[d], np.repeat(c2col[d][None], 3, axis=0), p, P.REPR_NTT) for d in range(D)]
    key = P.SecretKey.from_coefficients(p, sk)
    return (lambda: P.api._decrypt_batch(p, cts, key, 0, return_noisy=True)[1]), want


@pytest.mark.parametrize("k,l,L,D", DECRYPT_SHAPE_CASES)
def test_decrypt_mac_shape_selected_launch_agrees_with_c_oracle(k, l, L, D):
    # the launch shape the shipped library picks (the others: tests/test_gpu_tuning.py)
    run, want = decrypt_mac_case(k, l, L, D)
    assert np.array_equal(run(), want)


@pytest.mark.parametrize("D", [1, 2, 4, 7])
def test_multi_dealer_encrypt_equals_separate_encrypts(D):
    # encrypt_all_party_shares (encryption.rs:253-286) with the shipped split: the integer-VALU form (several
    # dealers per pass over B-hat) below 3 dealers, the matrix cores from 3 up (VALU form forced everywhere:
    # tests/test_gpu_tuning.py)
    multi_dealer_case(D)


def multi_dealer_case(D):
    n, k, l, moduli = 13, 9, 8, M.bench_moduli(4)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    rows = [[(d * 100 + j) for j in range(1, n + 1)] for d in range(D)]
    seeds = [P.api._dealer_seed(SEED, d) for d in range(D)]
    for repr in (P.REPR_NTT, P.REPR_POWER):
        many = P.encrypt_many(rows, gpk, seeds, repr)
        assert len(many) == D
        for d in range(D):
            one = P.encrypt(rows[d], gpk, seeds[d], repr=repr)
            assert np.array_equal(many[d].c1, one.c1) and np.array_equal(many[d].c2, one.c2)
    with pytest.raises(P.PvwError):
        P.encrypt_many([[1, 2, 3]], gpk, seeds[:1])


@pytest.mark.parametrize("n,k,l,L,D", [
    (13, 9, 8, 4, 9),         # ragged: k not a multiple of 4, rows not a multiple of 32, one partial vector group
    (70, 40, 8, 3, 16),       # more than two row tiles in the B section
    (10, 6, 16, 3, 21),       # l = 16, two passes of 16 + 5 dealers
    (5, 12, 32, 2, 8),        # l = 32
    (200, 256, 8, 17, 8),     # config-3 geometry (k=256, 17 limbs) at a small party count
    (100, 256, 8, 3, 40),     # k = 256: fully unrolled chunk loop, three batches (16 + 16 + 8) in one launch
    (40, 512, 16, 2, 17),     # k = 512: the 16-chunk unrolled form, one full batch + one dealer
    (6, 24, 64, 2, 9),        # l = 64
    (9, 8, 8, 3, 130),        # more dealers than one launch takes (128)
    (20, 528, 8, 2, 40),      # k > 512 in the wide form: unbiased integer recombination
    (37, 16, 8, 2, 33),       # the smallest k the wide form takes (two stages), ragged rows, three batches
])
def test_digit_gemm_multi_dealer_equals_separate_encrypts(n, k, l, L, D):
    # >= 3 dealers take the matrix-core path (gemm_digits_kernel): i8 MFMA over byte-folded operands
    digit_gemm_case(n, k, l, M.bench_moduli(L) if l <= 32 else primes_1mod(128, L), D)


@pytest.mark.parametrize("n,k,l,L,D", [
    (37, 64, 8, 4, 5),        # the smallest k of the 7-byte form (14 K tiles), one partial vector group, ragged rows
    (9, 256, 8, 2, 17),       # 56 K tiles, one full batch + one dealer: the wide form
    (70, 128, 8, 3, 33),      # three batches in one launch
    (10, 64, 16, 4, 21),      # l = 16
    (20, 576, 8, 2, 40),      # k > 512: unbiased integer recombination
    (5, 1024, 8, 4, 9),       # the reference's own 128-bit set (k = 1024): 224 K tiles, rolled chunk loop
])
def test_digit_gemm_seven_byte_contraction(n, k, l, L, D):
    # every modulus below 2^56 and k a multiple of 64: byte 7 of every matrix element is zero and is left out of the
    # contraction (gemm_ktiles: 7 K tiles per 32 terms instead of 8; mftile7_kernel / vec_digits7_kernel) -- the reference's
    # own 56-bit chain (examples/pvw_valid_dec.rs:40-45) against separate encrypts and the C restatement
    digit_gemm_case(n, k, l, EXAMPLE_MODULI[:L], D)


def digit_gemm_case(n, k, l, moduli, D):
    L = len(moduli)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    rng = np.random.default_rng(D)
    rows = [[int(x) for x in rng.integers(0, 1 << 63, size=n, dtype=np.uint64)] for _ in range(D)]
    rows[0][0] = (1 << 64) - 5
    seeds = [P.api._dealer_seed(SEED, d) for d in range(D)]
    many = P.encrypt_many(rows, gpk, seeds)
    for d in range(D):
        one = P.encrypt(rows[d], gpk, seeds[d])
        assert np.array_equal(many[d].c1, one.c1), f"c1 dealer {d}"
        assert np.array_equal(many[d].c2, one.c2), f"c2 dealer {d}"
    # ... and against the C restatement itself (not only the single-dealer HIP path): first, middle and last dealer
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(SEED, M.DOM_CRS, 0, k * k).reshape(k, k, L, l)
    b_hat = orc.fill_uniform(SEED, M.DOM_PK, 0, n * k).reshape(n, k, L, l)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    for d in sorted({0, D // 2, D - 1}):
        r = O.sample_cbd(seeds[d], M.DOM_R, 0, k, l, 0.5)
        e1 = O.sample_uniform(seeds[d], M.DOM_E1, 0, k, l, 100)
        e2 = O.sample_uniform(seeds[d], M.DOM_E2, 0, n, l, 200)
        c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(rows[d], dtype=np.uint64), r, e1, e2)
        assert np.array_equal(many[d].c1, c1o) and np.array_equal(many[d].c2, c2o), f"dealer {d} vs oracle"


@pytest.mark.parametrize("n,k,l,L,D", [(64, 256, 8, 2, 20), (40, 512, 8, 2, 17), (33, 512, 16, 2, 18)])
def test_digit_gemm_extreme_matrix_bytes_against_c_oracle(n, k, l, L, D):
    # The digit GEMM feeds the matrix elements to the i8 MFMA as raw bytes offset by -128 and recombines biased
    # accumulators in f64 (exact while |half-sum| < 2^51, i.e. k <= 512): matrices made of the byte patterns that
    # push the partial sums to their extremes -- all bytes 0x00 (-128 after the offset), q - 1 and 0x..ffff (+127),
    # 0x80.. (0), alternating -- must still give the oracle's ciphertexts (crs.rs:188-201, encryption.rs:177-200)
    digit_gemm_extreme_case(n, k, l, M.bench_moduli(L), D)


@pytest.mark.parametrize("n,k,l,L,D", [(64, 256, 8, 2, 20), (40, 512, 8, 2, 17), (33, 512, 16, 2, 18)])
def test_digit_gemm_seven_byte_extreme_matrix_bytes(n, k, l, L, D):
    # the same patterns (cut to residues below the 56-bit moduli) through the 7-byte contraction
    digit_gemm_extreme_case(n, k, l, EXAMPLE_MODULI[:L], D)


@pytest.mark.parametrize("moduli", [M.bench_moduli(2), EXAMPLE_MODULI[:2]], ids=["61-bit: 8-byte", "56-bit: 7-byte"])
def test_digit_gemm_extreme_matrix_bytes_kept_raw(moduli):
    # the same byte patterns kept as the raw words they are (0xFF.., 0x80.., ... >= q): a word w means w mod q, so the
    # ciphertexts must be the oracle's on the reduced matrices (the 7-byte operand holds 7 bytes of the REDUCED word)
    digit_gemm_extreme_case(64, 256, 8, moduli, 20, raw=True)


def digit_gemm_extreme_case(n, k, l, moduli, D, raw=False):
    L = len(moduli)
    p = build_params(n, k, l, moduli)
    rng = np.random.default_rng(k + l)
    q = np.array(moduli, dtype=np.uint64)[None, None, :, None]

    def patterned(rows):
        m = np.empty((rows, k, L, l), dtype=np.uint64)
        pats = [0, 0xFFFFFFFFFFFFFFFF, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0x00FF00FF00FF00FF, 0xFF00FF00FF00FF00,
                0x0000000000000001, 0x8000000000000000]
        for i in range(rows):
            if i % 3 == 2:
                m[i] = rng.integers(0, 1 << 61, size=(k, L, l), dtype=np.uint64)
            else:
                m[i] = np.uint64(pats[(i // 3 + i) % len(pats)])
        m[0] = 0
        m[1 % rows] = np.uint64(0xFFFFFFFFFFFFFFFF)
        if raw:
            return m
        bits = np.uint64(max(moduli).bit_length())
        return np.minimum(m % (np.uint64(1) << bits), q - np.uint64(1))   # residues below q with the byte patterns intact

    a_hat, b_hat = patterned(k), patterned(n)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.from_polynomials(p, a_hat, P.REPR_NTT))
    gpk.load_rows(0, b_hat, P.REPR_NTT)
    if raw:
        assert (a_hat >= q).any() and (b_hat >= q).any()
        a_hat, b_hat = a_hat % q, b_hat % q                              # what the oracle takes
    rows = [[int(x) for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)] for _ in range(D)]
    seeds = [P.api._dealer_seed(SEED, d) for d in range(D)]
    many = P.encrypt_many(rows, gpk, seeds)
    orc = O.Oracle(moduli, l)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    for d in sorted({0, 1, D // 2, D - 1}):
        r = O.sample_cbd(seeds[d], M.DOM_R, 0, k, l, 0.5)
        e1 = O.sample_uniform(seeds[d], M.DOM_E1, 0, k, l, 100)
        e2 = O.sample_uniform(seeds[d], M.DOM_E2, 0, n, l, 200)
        c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(rows[d], dtype=np.uint64), r, e1, e2)
        assert np.array_equal(many[d].c1, c1o), f"c1 dealer {d}"
        assert np.array_equal(many[d].c2, c2o), f"c2 dealer {d}"


@pytest.mark.parametrize("moduli", [M.bench_moduli(3), EXAMPLE_MODULI[:3]], ids=["61-bit: 8-byte contraction", "56-bit: 7-byte contraction"])
def test_digit_gemm_repeats_are_bit_identical(moduli):
    # The wide digit GEMM keeps LDS-DMA stages in flight across raw barriers (two wave groups half a stage apart): a
    # misplaced wait would show as a rare wrong tile, not as a wrong algorithm.  Same call 40 times, every result
    # equal to the first (tools/gemm_stress.py runs 2000 repeats at the bench sizes); the first is checked against
    # the oracle by the tests above.
    n, k, l, D = 600, 256, 8, 40
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    rows = [[(d * 7919 + j) for j in range(n)] for d in range(D)]
    seeds = [P.api._dealer_seed(SEED, d) for d in range(D)]
    first = P.encrypt_many(rows, gpk, seeds)
    for _ in range(40):
        again = P.encrypt_many(rows, gpk, seeds)
        assert all(np.array_equal(a.c1, b.c1) and np.array_equal(a.c2, b.c2) for a, b in zip(again, first))


def test_multi_dealer_encrypt_l16_and_sharded():
    n, k, l, moduli = 10, 6, 16, TEST_MODULI
    full = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(full, SEED))
    gpk.fill_uniform(SEED)
    rows = [[(d * 100 + j) for j in range(1, n + 1)] for d in range(n)]
    cts = P.encrypt_all_party_shares(rows, gpk, SEED)
    ps = build_params(n, k, l, moduli, shard=(3, 8, 2, 5))
    g2 = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(ps, SEED))
    g2.fill_uniform(SEED)
    part = P.encrypt_all_party_shares(rows, g2, SEED)
    for d in range(n):
        assert np.array_equal(part[d].c1[2:5], cts[d].c1[2:5]) and np.array_equal(part[d].c2[3:8], cts[d].c2[3:8])
        assert not part[d].c1[:2].any() and not part[d].c2[8:].any()


def mixed_width_moduli(count):
    # alternating 61-bit and 40-bit primes (= 1 mod 64): an earlier modulus more than twice a later one, so a mixed-radix
    # digit of the decode's short cut does not reduce to the next modulus with one subtraction
    wide, narrow = primes_1mod(64, (count + 1) // 2), primes_1mod(64, count // 2, top=1 << 40)
    return [wide[i // 2] if i % 2 == 0 else narrow[i // 2] for i in range(count)]


# which of the decode's short cuts the sets below reach (DecodeTables: gar_n / sc_on / hs_on): one modulus: none; the 36/37-bit
# test chain: candidates only (Q below 194 bits); the bench chains at l = 8 / 16 (Delta of 130 bits, three-word 2 Delta)
# and 17 limbs at l = 16 (Delta of 65 bits, two words): all of them; l = 64 over 5 limbs (Delta of 5 bits, one word):
# the chain at once but noise_{l-1} from the lifted Horner value; mixed widths: all, with full reductions between the digits
@pytest.mark.parametrize("l,moduli", [(8, [0xFFFFEE001]), (8, TEST_MODULI), (32, TEST_MODULI), (8, M.bench_moduli(17)),
                                      (16, M.bench_moduli(34)), (64, primes_1mod(128, 5)), (16, M.bench_moduli(17)),
                                      (8, mixed_width_moduli(12)), (8, mixed_width_moduli(5))])
def test_device_decode_matches_model(l, moduli):
    device_decode_case(l, moduli, lambda variant: None, (0,))


def device_decode_case(l, moduli, select_variant, variants):
    # decode_scalar_pvw_rns (decryption.rs:10-58) on the device, fixed-width integers
    p = build_params(3, 4, l, moduli)
    m = M.Params(3, 4, l, moduli)
    cases = decode_cases(l, moduli)
    arr = np.array([[[c % q for c in z] for q in moduli] for z in cases], dtype=np.uint64)
    want = [M.decode_scalar_pvw(z, m) for z in cases]
    assert want == P.decode_scalar_pvw_host(p, arr)
    # the shipped library picks the form by shape (lifted chain, 4 waves per ciphertext, for every Q here); the
    # tuning build walks the others: 2 / 8 waves, one wave per ciphertext with an RNS round trip per step, one thread
    for variant in variants:
        select_variant(variant)
        assert P.decode_scalar_pvw(p, arr) == want, variant


def test_concurrent_encrypt_calls_on_one_context():
    # the reference calls encrypt concurrently from rayon workers (encryption.rs:277-283); host-buffer
    # ABI calls must be safe to issue concurrently on one context (ctypes releases the GIL)
    import threading
    n, k, l, moduli = 40, 16, 8, M.bench_moduli(3)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    jobs = [([(d * 100 + j) for j in range(n)], P.api._dealer_seed(SEED, d)) for d in range(24)]
    want = [P.encrypt(sc, gpk, sd) for sc, sd in jobs]
    got = [None] * len(jobs)
    errs = []

    def work(idx):
        try:
            for i in range(idx, len(jobs), 6):
                got[i] = P.encrypt(jobs[i][0], gpk, jobs[i][1])
        except Exception as e:          # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs
    for a, b in zip(got, want):
        assert np.array_equal(a.c1, b.c1) and np.array_equal(a.c2, b.c2)
    sk = P.SecretKey.random(p, SEED, 0)
    assert P.decrypt_party_shares(want[:n], sk, 0) == P.decrypt_party_shares(got[:n], sk, 0) if len(want) >= n else True


def test_mfma_i8_operand_maps():
    # exact-integer check of the lane maps the digit-GEMM kernels rely on (asymmetric operands)
    import ctypes as C
    p = build_params(3, 4, 8, TEST_MODULI)
    rng = np.random.default_rng(5)
    a = rng.integers(-128, 128, size=(32, 32), dtype=np.int8)
    b = rng.integers(-128, 128, size=(32, 32), dtype=np.int8)
    out = np.zeros((32, 32), dtype=np.int32)
    p._call("pvw_selftest_mfma_i8", a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out, a.astype(np.int32) @ b.astype(np.int32))


def test_sharded_contexts_match_unsharded():
    # one process per GPU holds rows [party_lo, party_hi) of B and [c1_lo, c1_hi) of A
    n, k, l, moduli = 21, 12, 8, M.bench_moduli(3)
    full = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(full, SEED))
    gpk.fill_uniform(SEED)
    scalars = [(i * 1000 + 1) % (1 << 32) for i in range(n)]
    ct = P.encrypt(scalars, gpk, SEED)
    c1 = np.zeros_like(ct.c1)
    c2 = np.zeros_like(ct.c2)
    world = 3
    for rank in range(world):
        lo, hi = n * rank // world, n * (rank + 1) // world
        clo, chi = k * rank // world, k * (rank + 1) // world
        ps = build_params(n, k, l, moduli, shard=(lo, hi, clo, chi))
        g = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(ps, SEED))
        g.fill_uniform(SEED)
        assert g.is_full()
        part = P.encrypt(scalars, g, SEED)
        assert not part.c1[:clo].any() and not part.c2[:lo].any()
        c1[clo:chi] = part.c1[clo:chi]
        c2[lo:hi] = part.c2[lo:hi]
    assert np.array_equal(c1, ct.c1) and np.array_equal(c2, ct.c2)


def test_config4_geometry_keygen_encrypt_decrypt():
    # BASELINE configs[3]/[4] geometry (k=512, l=16, 34 limbs = 2074-bit Q) at a party count the CPU
    # oracle finishes in seconds: keygen, encrypt and batched decrypt bit-exact vs the C restatement,
    # then the full round trip through the on-device decode.
    n, k, l, L = 24, 512, 16, 34
    moduli = M.bench_moduli(L)
    p = build_params(n, k, l, moduli)
    assert p.q_total().bit_length() == 2074 and p.verify_correctness_condition()
    seed = bytes([0xC4]) * 32
    crs = P.PvwCrs.new_deterministic(p, seed)
    gpk = P.GlobalPublicKey.new(crs)
    parties = [P.Party.new(i, p, seed) for i in range(n)]
    gpk.generate_all_party_keys(parties, seed)
    orc = O.Oracle(moduli, l)
    a_hat = crs.matrix(P.REPR_NTT)
    assert np.array_equal(a_hat, orc.fill_uniform(seed, M.DOM_CRS, 0, k * k).reshape(k, k, L, l))
    sk = np.stack([pt.secret_key.secret_coeffs for pt in parties])
    assert np.array_equal(sk, O.sample_cbd(seed, M.DOM_SK, 0, n * k, l, 0.5).reshape(n, k, l))
    ek = O.sample_uniform(seed, M.DOM_EKEY, 0, n * k, l, 100).reshape(n, k, l)
    b_hat = gpk.matrix(repr=P.REPR_NTT)
    assert np.array_equal(b_hat, orc.keygen(a_hat, sk, ek))
    scalars = np.array([(i * 1000 + 1) % (1 << 32) for i in range(n)], dtype=np.uint64)
    ct = P.encrypt(scalars, gpk, seed)
    r = O.sample_cbd(seed, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(seed, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(seed, M.DOM_E2, 0, n, l, 200)
    c1o, c2o = orc.encrypt(a_hat, b_hat, p.gadget_polynomial(P.REPR_NTT), scalars, r, e1, e2)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    got = []
    for i in range(n):
        vals, noisy = P.api._decrypt_batch(p, [ct], parties[i].secret_key, i, return_noisy=True)
        assert np.array_equal(noisy, orc.decrypt_noisy(sk[i], ct.c1[None], ct.c2[i][None]))
        got.append(vals[0])
    assert got == [int(x) for x in scalars]


@pytest.mark.parametrize("case", range(int(os.environ.get("PVW_RANDOM_CASES", "12"))))   # soak: PVW_RANDOM_CASES=80
def test_random_geometries_full_pipeline_against_c_oracle(case):
    # seeded random (n, k, l, L, D, variance, bounds): key generation, single- and multi-dealer encrypt, batched
    # decrypt and decode, each against the C restatement / the big-integer model -- the reference's own tests
    # walk a handful of fixed geometries (tests/crypto.rs, tests/keys.rs); this widens them
    rng = np.random.default_rng(1000 + case)
    for _ in range(50):                      # redraw until the reference's correctness gate (parameters.rs:510-551) passes
        l = int(rng.choice([8, 8, 16, 32]))
        L = int(rng.integers(1, 7))
        k = int(rng.integers(1, 70))
        n = int(rng.integers(1, 60))
        D = int(rng.integers(1, 40))
        variance = float(rng.choice([0.5, 1.0, 2.0, 3.0]))
        b1, b2 = int(rng.integers(1, 500)), int(rng.integers(1, 5000))
        moduli = M.bench_moduli(L)
        p = build_params(n, k, l, moduli, variance, (b1, b2))
        if p.verify_correctness_condition():
            break
    else:
        pytest.fail("no geometry passed the correctness gate")
    seed = bytes([17 + case]) * 32
    orc = O.Oracle(moduli, l)
    crs = P.PvwCrs.new_deterministic(p, seed)
    a_hat = crs.matrix(P.REPR_NTT)
    gpk = P.GlobalPublicKey.new(crs)
    parties = [P.Party.new(i, p, seed) for i in range(n)]
    gpk.generate_all_party_keys(parties, seed)
    sk = O.sample_cbd(seed, M.DOM_SK, 0, n * k, l, variance).reshape(n, k, l)
    ek = O.sample_uniform(seed, M.DOM_EKEY, 0, n * k, l, b1).reshape(n, k, l)
    b_hat = gpk.matrix(repr=P.REPR_NTT)
    assert np.array_equal(b_hat, orc.keygen(a_hat, sk, ek)), "keygen"
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    rows = [[int(x) for x in rng.integers(0, 1 << 32, size=n, dtype=np.uint64)] for _ in range(D)]
    seeds = [P.api._dealer_seed(seed, d) for d in range(D)]
    many = P.encrypt_many(rows, gpk, seeds)
    for d in (0, D // 2, D - 1):
        r = O.sample_cbd(seeds[d], M.DOM_R, 0, k, l, variance)
        e1 = O.sample_uniform(seeds[d], M.DOM_E1, 0, k, l, b1)
        e2 = O.sample_uniform(seeds[d], M.DOM_E2, 0, n, l, b2)
        c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(rows[d], dtype=np.uint64), r, e1, e2)
        assert np.array_equal(many[d].c1, c1o) and np.array_equal(many[d].c2, c2o), f"multi-dealer encrypt {d}"
        one = P.encrypt(rows[d], gpk, seeds[d])
        assert np.array_equal(one.c1, c1o) and np.array_equal(one.c2, c2o), f"encrypt {d}"
    # party i decrypts its share from every dealer
    mparams = M.Params(n, k, l, moduli)
    for i in (0, n - 1):
        vals, noisy = P.api._decrypt_batch(p, many, parties[i].secret_key, i, return_noisy=True)
        c1s = np.stack([ct.c1 for ct in many])
        c2col = np.stack([ct.c2[i] for ct in many])
        want_noisy = orc.decrypt_noisy(sk[i], c1s, c2col)
        assert np.array_equal(noisy, want_noisy), f"decrypt party {i}"
        lifted = [rns_to_ring(want_noisy[d], moduli) for d in range(D)]
        assert vals == [M.decode_scalar_pvw(z, mparams) for z in lifted], f"decode party {i}"
        # Recovery of the scalars is a property of the scheme, not of this implementation (device == model above).
        # The gate does not look at the message size, so only geometries whose Delta exceeds the 32-bit scalars
        # are held to the reference's own >= 95 % (tests/crypto.rs:295-304).
        if mparams.delta.bit_length() > 34:
            assert sum(v == rows[d][i] for d, v in enumerate(vals)) >= 0.95 * D - 1


@pytest.mark.parametrize("n,k,l,L", [(150, 256, 8, 2), (70, 9, 8, 3), (1100, 32, 16, 2),
                                            (3100, 8, 8, 2),      # four 1024-party chunks: both key buffers reused
                                            (40, 24, 8, 2),       # below 64 parties: transposed CRS as the streamed operand
                                            (5, 12, 8, 2),        # below 8: four per pass on the integer VALU
                                            (70, 12, 32, 2),      # l = 32: 16 lanes share out a row in the fused finish pass
                                            (66, 528, 8, 2)])     # k > 512: wide GEMM with the unbiased integer recombination
def test_batched_keygen_super_groups_against_c_oracle(n, k, l, L):
    # pvw_keygen on the matrix cores (public_key.rs:111-147, crs.rs:138-171) against the C restatement, with seeded
    # and with explicit key errors.  From 64 parties up the parties are the GEMM rows and the CRS columns are
    # digitised once per call (also: ragged k, more than one 1024-party chunk); the earlier form (transposed CRS
    # streamed, super-groups of 128 secret keys digitised) serves 8..63 parties here and every size in
    # tests/test_gpu_tuning.py (PVW_KEYGEN_SWAP=0)
    batched_keygen_case(n, k, l, L)


def batched_keygen_case(n, k, l, L, moduli=None):
    moduli = moduli or M.bench_moduli(L)
    p = build_params(n, k, l, moduli)
    seed = bytes([0x5A]) * 32
    crs = P.PvwCrs.new_deterministic(p, seed)
    orc = O.Oracle(moduli, l)
    a_hat = crs.matrix(P.REPR_NTT)
    sk = O.sample_cbd(seed, M.DOM_SK, 0, n * k, l, 0.5).reshape(n, k, l)
    ek = O.sample_uniform(seed, M.DOM_EKEY, 0, n * k, l, 100).reshape(n, k, l)
    want = orc.keygen(a_hat, sk, ek)
    gpk = P.GlobalPublicKey.new(crs)
    parties = [P.Party.new(i, p, seed) for i in range(n)]
    gpk.generate_all_party_keys(parties, seed)
    assert np.array_equal(gpk.matrix(repr=P.REPR_NTT), want)
    gpk2 = P.GlobalPublicKey.new(crs)
    gpk2.generate_with_errors(0, sk, ek)
    assert np.array_equal(gpk2.matrix(repr=P.REPR_NTT), want)


def test_config2_full_size_against_c_oracle():
    # BASELINE.json configs[1]: n=1024, k=256, l=8, 17 limbs (1037-bit Q), bit-exact vs the CPU path
    n, k, l, L = 1024, 256, 8, 17
    moduli = M.bench_moduli(L)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, bytes([0xA]) * 32))
    gpk.fill_uniform(bytes([0xB]) * 32)
    scalars = np.array([(i * 1000 + 1) % (1 << 32) for i in range(n)], dtype=np.uint64)
    ct = P.encrypt(scalars, gpk, SEED)
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(bytes([0xA]) * 32, M.DOM_CRS, 0, k * k).reshape(k, k, L, l)
    b_hat = orc.fill_uniform(bytes([0xB]) * 32, M.DOM_PK, 0, n * k).reshape(n, k, L, l)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(SEED, M.DOM_E2, 0, n, l, 200)
    c1o, c2o = orc.encrypt(a_hat, b_hat, p.gadget_polynomial(P.REPR_NTT), scalars, r, e1, e2)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    # linearity property at full size: Enc(m; r,e) - Enc(m'; r,e) = (m - m') * g, limb-wise
    ct2 = P.encrypt(scalars + np.uint64(5), gpk, SEED, repr=P.REPR_POWER)
    ct1 = P.encrypt(scalars, gpk, SEED, repr=P.REPR_POWER)
    g = p.gadget_polynomial(P.REPR_POWER)
    for i, q in enumerate(moduli):
        diff = (ct2.c2[:, i].astype(object) - ct1.c2[:, i].astype(object)) % q
        want = (5 * g[i].astype(object)) % q
        assert (diff == want[None, :]).all()
    assert np.array_equal(ct1.c1, ct2.c1)


def test_config4_full_size_sampled_rows_against_c_oracle():
    # BASELINE.json configs[3] on ONE GPU at full size: n = 16384, k = 512, l = 16, 34 limbs (2074-bit Q); B-hat
    # is 36.5 GB.  All of c1 and three windows of c2 rows (first, middle, last) against the C restatement on the
    # same synthetic A-hat / B-hat: a size the 32-bit index arithmetic of a kernel would not survive by accident.
    n, k, l, L = 16384, 512, 16, 34
    moduli = M.bench_moduli(L)
    p = build_params(n, k, l, moduli)
    sa, sb = bytes([0xA]) * 32, bytes([0xB]) * 32
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, sa))
    gpk.fill_uniform(sb)
    scalars = np.array([(i * 1000 + 1) % (1 << 32) for i in range(n)], dtype=np.uint64)
    ct = P.encrypt(scalars, gpk, SEED)
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(sa, M.DOM_CRS, 0, k * k).reshape(k, k, L, l)
    r = O.sample_cbd(SEED, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(SEED, M.DOM_E1, 0, k, l, 100)
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    for lo in (0, n // 2 - 3, n - 8):
        rows = 8
        b_sub = orc.fill_uniform(sb, M.DOM_PK, lo * k, rows * k).reshape(rows, k, L, l)
        assert np.array_equal(gpk.matrix(lo, lo + rows, P.REPR_NTT), b_sub)
        e2 = O.sample_uniform(SEED, M.DOM_E2, lo, rows, l, 200)
        c1o, c2o = orc.encrypt(a_hat, b_sub, g_hat, scalars[lo:lo + rows], r, e1, e2)
        assert np.array_equal(ct.c2[lo:lo + rows], c2o), f"c2 rows {lo}.."
        if lo == 0:
            assert np.array_equal(ct.c1, c1o), "c1"



def _bench_config_against_c_oracle(n):
    """one encrypt at a BASELINE geometry (k=256, l=8, 17 limbs) in full against the C restatement, plus the
    size-independent linearity property"""
    from pvw_rs_amd import workloads as W
    k, l, L = 256, 8, 17
    moduli = W.bench_moduli(L)
    p = build_params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, W.SEED_A))
    gpk.fill_uniform(W.SEED_B)
    scalars = np.array(W.scalars(n), dtype=np.uint64)
    ct = P.encrypt(scalars, gpk, W.SEED_ENC)
    orc = O.Oracle(moduli, l)
    a_hat = orc.fill_uniform(W.SEED_A, M.DOM_CRS, 0, k * k).reshape(k, k, L, l)
    b_hat = orc.fill_uniform(W.SEED_B, M.DOM_PK, 0, n * k).reshape(n, k, L, l)
    r = O.sample_cbd(W.SEED_ENC, M.DOM_R, 0, k, l, 0.5)
    e1 = O.sample_uniform(W.SEED_ENC, M.DOM_E1, 0, k, l, 100)
    e2 = O.sample_uniform(W.SEED_ENC, M.DOM_E2, 0, n, l, 200)
    c1o, c2o = orc.encrypt(a_hat, b_hat, p.gadget_polynomial(P.REPR_NTT), scalars, r, e1, e2)
    assert np.array_equal(ct.c1, c1o) and np.array_equal(ct.c2, c2o)
    ct5 = P.encrypt(scalars + np.uint64(5), gpk, W.SEED_ENC)          # Enc(m + 5) - Enc(m) = 5 * g-hat, limb-wise
    g = p.gadget_polynomial(P.REPR_NTT)
    for i, q in enumerate(moduli):
        diff = (ct5.c2[:, i].astype(object) - ct.c2[:, i].astype(object)) % q
        assert (diff == ((5 * g[i].astype(object)) % q)[None, :]).all()
    assert np.array_equal(ct5.c1, ct.c1)


def test_config1_plumbing_size_against_c_oracle():
    # BASELINE.json configs[0]: n=16, k=256, l=8, 1037-bit q -- c1 (k^2 MACs) dominates, one row block of B
    _bench_config_against_c_oracle(16)


def test_config3_full_size_against_c_oracle():
    # BASELINE.json configs[2], the headline: n=4096, k=256, l=8, 17 limbs -- every c1 and c2 polynomial
    _bench_config_against_c_oracle(4096)


def test_reference_128_bit_parameter_set_full_pipeline():
    # the reference's one "128-bit" set at full size (examples/pvw_valid_dec.rs:40-52; tests/params.rs:253-274
    # sweeps k up to 1024): n=5, k=1024, l=8, 4 x 56-bit moduli, variance 10, bounds (1, 1172385).
    # keygen -> encrypt (one dealer: mac_rows; five dealers: the rolled digit GEMM at k=1024) -> decrypt -> decode,
    # each stage against the C restatement / the big-integer model
    n, k, l, moduli, variance, b1, b2 = 5, 1024, 8, EXAMPLE_MODULI, 10.0, 1, 1172385
    L = len(moduli)
    p = build_params(n, k, l, moduli, variance, (b1, b2))
    assert p.verify_correctness_condition()
    seed = bytes([0x80]) * 32
    orc = O.Oracle(moduli, l)
    crs = P.PvwCrs.new_deterministic(p, seed)
    a_hat = crs.matrix(P.REPR_NTT)
    assert np.array_equal(a_hat, orc.fill_uniform(seed, M.DOM_CRS, 0, k * k).reshape(k, k, L, l))
    gpk = P.GlobalPublicKey.new(crs)
    parties = [P.Party.new(i, p, seed) for i in range(n)]
    gpk.generate_all_party_keys(parties, seed)
    sk = O.sample_cbd(seed, M.DOM_SK, 0, n * k, l, variance).reshape(n, k, l)
    assert np.array_equal(np.stack([pt.secret_key.secret_coeffs for pt in parties]), sk)
    assert np.abs(sk).max() > 2                                         # variance 10: the wide CBD branch (uniform.rs:45-68)
    ek = O.sample_uniform(seed, M.DOM_EKEY, 0, n * k, l, b1).reshape(n, k, l)
    b_hat = gpk.matrix(repr=P.REPR_NTT)
    assert np.array_equal(b_hat, orc.keygen(a_hat, sk, ek)), "keygen"
    g_hat = p.gadget_polynomial(P.REPR_NTT)
    rows = [[dealer * 100 + j for j in range(1, n + 1)] for dealer in range(n)]   # pvw_valid_dec.rs:117-124 pattern
    cts = P.encrypt_all_party_shares(rows, gpk, seed)                   # 5 dealers -> gemm_digits, rolled K loop
    for d in range(n):
        sd = P.api._dealer_seed(seed, d)
        r = O.sample_cbd(sd, M.DOM_R, 0, k, l, variance)
        e1 = O.sample_uniform(sd, M.DOM_E1, 0, k, l, b1)
        e2 = O.sample_uniform(sd, M.DOM_E2, 0, n, l, b2)
        c1o, c2o = orc.encrypt(a_hat, b_hat, g_hat, np.array(rows[d], dtype=np.uint64), r, e1, e2)
        assert np.array_equal(cts[d].c1, c1o) and np.array_equal(cts[d].c2, c2o), f"multi-dealer encrypt {d}"
        one = P.encrypt(rows[d], gpk, sd)                               # mac_rows at k = 1024
        assert np.array_equal(one.c1, c1o) and np.array_equal(one.c2, c2o), f"encrypt {d}"
    mparams = M.Params(n, k, l, moduli, variance, b1, b2)
    ok = total = 0
    for i in range(n):
        vals, noisy = P.api._decrypt_batch(p, cts, parties[i].secret_key, i, return_noisy=True)
        c1s = np.stack([ct.c1 for ct in cts])
        c2col = np.stack([ct.c2[i] for ct in cts])
        want_noisy = orc.decrypt_noisy(sk[i], c1s, c2col)
        assert np.array_equal(noisy, want_noisy), f"decrypt party {i}"
        assert vals == [M.decode_scalar_pvw(rns_to_ring(want_noisy[d], moduli), mparams) for d in range(n)], f"decode {i}"
        ok += sum(v == rows[d][i] for d, v in enumerate(vals))
        total += n
    assert ok >= 0.95 * total                                           # tests/crypto.rs:295-304


def test_key_material_is_wiped_from_device_scratch():
    # SecretKey is Zeroize + ZeroizeOnDrop in the reference (secret_key.rs:20-30): after key generation and
    # decryption no device region that held sk coefficients, NTT(sk), key errors or their tiled / digitised copies
    # reads anything but zero (pvw_selftest_secret_residue scans what the calls declared secret + every s-hat block)
    for n, k in ((150, 32), (20, 24), (5, 12)):                        # swapped GEMM form, transposed-CRS form, VALU form
        p = build_params(n, k, 8, M.bench_moduli(3))
        gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
        parties = [P.Party.new(i, p, SEED) for i in range(n)]
        assert P.api._secret_residue(p)[0] == 0                         # SecretKey::random staging
        gpk.generate_all_party_keys(parties, SEED)
        nz, scanned = P.api._secret_residue(p)
        assert nz == 0 and scanned > n * k * 8, (n, k, nz, scanned)
        ct = P.encrypt(list(range(n)), gpk, SEED)
        got = P.decrypt_party_value(ct, parties[1].secret_key, 1)
        assert got == 1
        nz, scanned = P.api._secret_residue(p)
        assert nz == 0 and scanned > 0, (n, k, nz)

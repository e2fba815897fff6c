"""CPU checks of the checked decode: each share's noise and whether its decode was lossy.  The host big-integer
implementation (pvw_decode_checked_host) and the fixed-width device algorithm run on the host (pvw_selftest_decode_checked)
against the contract restated here from the model's decode, on boundary inputs at six parameter sets; noise_bound() against
the reference's total_bound."""
import math

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import api
from _util import EXAMPLE_MODULI, MIXED_CHAINS, TEST_MODULI, decode_cases, primes_1mod

U64 = (1 << 64) - 1

# (moduli, l): a small Q (two ~36-bit limbs, Delta * 2^64 > Q: every step of the device recurrence reduces), the 128-bit
# set of examples/pvw_valid_dec.rs, the bench chain at l = 16 / 32, l = 64 and a chain that starts with a tiny modulus
SETS = {
    "smallQ_l8": (TEST_MODULI[:2], 8),
    "test3_l8": (TEST_MODULI, 8),
    "example128_l8": (EXAMPLE_MODULI, 8),
    "bench5_l16": (M.bench_moduli(5), 16),
    "bench3_l32": (M.bench_moduli(3), 32),
    "l64": (primes_1mod(128, 3), 64),
    "tiny_first_l8": (MIXED_CHAINS["tiny_first"], 8),
}


def _params(moduli, l, n=3, k=4, bounds=None):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if bounds:
        b = b.set_error_bounds(*bounds)
    return b.build()


def plain_of(z_ints, m):
    """the model's decode (oracle/pvw_model.py decode_scalar_pvw) up to the plaintext P, before the u64 conversion"""
    Q, l, D = m.Q, m.l, m.delta
    z = [M.center(v % Q, Q) for v in z_ints]
    tmp = [(z[i] * D - z[i + 1]) % Q for i in range(l - 1)]
    last = tmp[0]
    for i in range(1, l - 1):
        last = (last * D + tmp[i]) % Q
    poly_const = M.center(last, Q)
    mod_const = M.center(m.delta_power_l_minus_1 % Q, Q)
    reduced = M.trem(poly_const, mod_const)
    half = M.tdiv(mod_const, 2)
    if reduced > half:
        reduced -= mod_const
    elif reduced < -half:
        reduced += mod_const
    noise = [0] * l
    noise[l - 1] = reduced % Q
    dc = M.center(D % Q, Q)
    for i in range(l - 2, -1, -1):
        p = M.center((noise[i + 1] - tmp[i]) % Q, Q)
        quo = 0 if dc == 0 else (M.tdiv(2 * p - dc, 2 * dc) if p < 0 else M.tdiv(2 * p + dc, 2 * dc))
        noise[i] = quo % Q
    return M.center((-z[0] - noise[0]) % Q, Q)


def expected(z_ints, m):
    """(out, noise, lossy) by the contract: residual_i = centre(-z_i - P Delta^i mod Q)"""
    Q, D = m.Q, m.delta
    p = plain_of(z_ints, m)
    res = [abs(M.center((-z_ints[i] - p * D ** i) % Q, Q)) for i in range(m.l)]
    return M.decode_scalar_pvw(z_ints, m), min(max(res), U64), not (0 <= p <= U64)


def checked_cases(m):
    """decode_cases plus inputs built around a chosen noise vector and plaintext"""
    Q, D, l = m.Q, m.delta, m.l
    rng = np.random.default_rng(7 * l + len(m.moduli))
    cases = decode_cases(l, m.moduli)
    top = m.delta_power_l_minus_1 // 2
    for amp in (0, 1, U64, 1 << 64, (1 << 64) + 1, top - 1, top, top + 1, Q // 2):
        for msg in (0, 5, -1000, -1001, 1 << 63, (1 << 63) + 5, U64, 1 << 64):
            for pos in (0, l - 1, l // 2):
                e = [int(x) for x in rng.integers(-3, 4, size=l)]
                e[pos] = amp if pos % 2 == 0 else -amp
                cases.append([(-(msg * D ** j) + e[j]) % Q for j in range(l)])
    return cases


def _rns(cases, moduli):
    return np.array([[[c % q for c in z] for q in moduli] for z in cases], dtype=np.uint64)


@pytest.mark.parametrize("name", sorted(SETS))
def test_checked_decode_host_and_device_algorithm_match_the_definition(name):
    moduli, l = SETS[name]
    p = _params(moduli, l)
    m = M.Params(3, 4, l, moduli)
    cases = checked_cases(m)
    noisy = _rns(cases, moduli)
    want = [expected(z, m) for z in cases]
    w_out = np.array([w[0] for w in want], dtype=np.uint64)
    w_noise = np.array([w[1] for w in want], dtype=np.uint64)
    w_lossy = np.array([w[2] for w in want])
    host = P.decode_scalar_pvw_checked_host(p, noisy)
    fixed = api._selftest_decode_checked(p, noisy)
    plain = np.array(P.decode_scalar_pvw_host(p, noisy), dtype=np.uint64)
    for tag, r in (("host", host), ("selftest", fixed)):
        assert np.array_equal(r.values, plain), tag
        assert np.array_equal(r.values, w_out), tag
        bad = np.nonzero(r.noise != w_noise)[0]
        assert len(bad) == 0, (tag, [(int(i), int(r.noise[i]), int(w_noise[i])) for i in bad[:5]])
        assert np.array_equal(r.lossy, w_lossy), tag
        assert np.all((r.status & ~np.uint32(P.DEC_LOSSY)) == 0), tag
    # the inputs reach every kind of report: exact small noise, lossy and not, and saturation wherever Q leaves room for it
    assert (w_noise < 1 << 20).any() and w_lossy.any() and (~w_lossy).any()
    assert (w_noise == U64).any() or m.Q.bit_length() < 80
    assert (w_noise > 1 << 40).any()


@pytest.mark.parametrize("name", ["smallQ_l8", "example128_l8", "bench5_l16"])
def test_unreduced_words_give_the_report_of_their_residues(name):
    moduli, l = SETS[name]
    p = _params(moduli, l)
    m = M.Params(3, 4, l, moduli)
    noisy = _rns(checked_cases(m)[::7], moduli)
    big = noisy.copy()
    for i, q in enumerate(moduli):                       # w + j q for the largest j that stays below 2^64
        j = (U64 - big[:, i, :].astype(object)) // q
        big[:, i, :] = (big[:, i, :].astype(object) + j * q).astype(np.uint64)
    assert (big != noisy).any()
    for fn in (P.decode_scalar_pvw_checked_host, api._selftest_decode_checked):
        a, b = fn(p, noisy), fn(p, big)
        assert np.array_equal(a.values, b.values) and np.array_equal(a.noise, b.noise) and np.array_equal(a.status, b.status)


def test_valid_is_not_lossy_and_within_the_bound():
    moduli, l = SETS["example128_l8"]
    p = _params(moduli, l)
    m = M.Params(3, 4, l, moduli)
    D, Q = m.delta, m.Q
    cases = [[(-(msg * D ** j) + (amp if j == 3 else 0)) % Q for j in range(l)]
             for msg, amp in ((7, 10), (7, 11), (-1001, 0), (1 << 64, 0))]
    r = P.decode_scalar_pvw_checked_host(p, _rns(cases, moduli), bound=10)
    assert list(r.noise) == [10, 11, 0, 0]
    assert list(r.lossy) == [False, False, True, True]
    assert list(r.valid) == [True, False, False, False]
    values, noise, lossy, valid = r
    assert list(values) == [7, 7, 0, 0]


def _total_bound(n, k, l, b1, b2):
    """parameters.rs:516-543 in f64, in the reference's order"""
    first = float(b2) * math.sqrt(float(n) * float(l)) * (1.0 + math.sqrt(float(n)))
    second = 2.0 * float(b1) * float(k) * float(l)
    third = 14.0 * float(b1) * math.sqrt(float(n) * float(k) * float(l))
    return first + second + third


@pytest.mark.parametrize("n,k,l,moduli,bounds", [
    (3, 4, 8, TEST_MODULI, None),
    (1024, 1024, 8, EXAMPLE_MODULI, (1, 1172385)),
    (5, 16, 8, TEST_MODULI, (3, 77)),
    (48, 32, 16, M.bench_moduli(5), (100, 200)),
    (7, 64, 64, primes_1mod(128, 3), (2 ** 31, 2 ** 32 - 1)),
])
def test_noise_bound_is_the_reference_total_bound(n, k, l, moduli, bounds):
    p = _params(moduli, l, n=n, k=k, bounds=bounds)
    t = math.floor(_total_bound(n, k, l, p.error_bound_1, p.error_bound_2))
    assert p.noise_bound() == min(t, U64)
    assert p.verify_correctness_condition() == (float(p.delta_power_l_minus_1()) > _total_bound(n, k, l, p.error_bound_1,
                                                                                                p.error_bound_2))

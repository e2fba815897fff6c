"""Shamir shares on the host side: pvw_shamir_shares_host against a restatement of the contract in Python
integers (coefficients from the model's ChaCha8 with the stream id and rejection rule of the contract, shares by pow and %),
pvw_shamir_reconstruct giving the secrets back from random subsets of t + 1 parties, the argument errors, and the mirrors.
No device compute here; the kernel and the fused deal are checked in tests/test_gpu_shamir.py.

The grid.  Every value the contract names appears: p in {smallest prime above n, 65537, the prime just above 2^31, 2^61 - 1,
the largest prime below 2^62}, degree in {0, 1, 2, a middle value, n - 1}, n in {3, 64, 100, 1000}, D in {1, 5, 130}, secrets
up to 2^64 - 1, explicit coefficients all p - 1.  The restatement costs D n t calls of pow, so the large values meet in
chosen combinations (CASES below) and not in the full product: n = 1000 with degree 999 at D = 1, D = 130 at n = 100."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import TEST_MODULI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS = 1
U64 = (1 << 64) - 1
DOM_SHAMIR = 9
NEW = ["pvw_shamir_shares_host", "pvw_shamir_shares_device", "pvw_shamir_shares", "pvw_deal_shares", "pvw_deal_shares_device",
       "pvw_deal_shares_rs", "pvw_deal_shares_rs_device", "pvw_shamir_reconstruct"]


def next_prime(x):
    x += 1
    while not M.is_prime(x):
        x += 1
    return x


def prev_prime(x):
    x -= 1
    while not M.is_prime(x):
        x -= 1
    return x


P31 = next_prime(1 << 31)              # 32 bits wide, just above half the range of a 32-bit draw: every other draw is rejected
P61 = (1 << 61) - 1
P62 = prev_prime(1 << 62)


def primes_for(n):
    return sorted({next_prime(n), 65537, P31, P61, P62})


def params(n):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(TEST_MODULI).build()


def seeds_for(D, tag=0):
    return [bytes((7 * d + 13 * i + tag) & 0xFF for i in range(32)) for d in range(D)]


def secrets_for(D, p, rng):
    """unreduced words: the extremes first, then any 64-bit word"""
    fixed = [U64, 0, p, p - 1, U64 - 1, 1 << 63]
    return [fixed[d] if d < len(fixed) else rng.getrandbits(64) for d in range(D)]


def restated_coeffs(seed, degree, p, stats=None):
    """a_j (j = 1..degree): the first accepted draw of the stream (seed, (DOM_SHAMIR << 32) | j): next_u64() >> clz(p), accepted
    when below p"""
    sh = 64 - p.bit_length()
    out = []
    for j in range(1, degree + 1):
        g = M.ChaChaRng(seed, DOM_SHAMIR, j)
        while True:
            v = g.next_u64() >> sh
            if v < p:
                break
            if stats is not None:
                stats["rejected"] += 1
        out.append(v)
    return out


def restated_shares(n, secrets, degree, p, seeds=None, coeffs=None, stats=None):
    rows = []
    for d, s in enumerate(secrets):
        a = [s % p] + ([c % p for c in coeffs[d]] if coeffs is not None else restated_coeffs(seeds[d], degree, p, stats))
        rows.append([sum(a[j] * pow(i + 1, j, p) for j in range(degree + 1)) % p for i in range(n)])
    return rows


# (n, D, degrees, primes): see the module docstring
CASES = [
    (3, 1, [0, 1, 2], primes_for(3)),
    (3, 5, [0, 1, 2], primes_for(3)),
    (64, 5, [0, 1, 2, 31, 63], primes_for(64)),
    (64, 1, [63], [next_prime(64), P62]),
    (100, 130, [2, 50, 99], [next_prime(100), P61]),
    (100, 5, [99], [65537, P31, P62]),
    (1000, 1, [999], [next_prime(1000), P62]),
    (1000, 5, [0, 1, 500], [P31]),
    (1000, 5, [2], [65537, P61]),
]


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name
    assert _ffi.DOM_SHAMIR == DOM_SHAMIR and "PVW_DOM_SHAMIR = 9" in header


@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_shares_equal_the_restatement_and_reconstruct(case):
    n, D, degrees, primes = CASES[case]
    prm = params(n)
    rng = random.Random(1000 + case)
    for p in primes:
        for t in degrees:
            secrets = secrets_for(D, p, rng)
            seeds = seeds_for(D, tag=t)
            stats = {"rejected": 0}
            want = restated_shares(n, secrets, t, p, seeds=seeds, stats=stats)
            got = P.shamir_shares(prm, secrets, t, p, seeds=seeds, host=True)
            assert got.tolist() == want, (n, D, t, p)
            if p == P31 and D * t >= 8:
                assert stats["rejected"] > 0, "the 32-bit prime must exercise the rejection rule"
            # several random subsets of t + 1 parties give every dealer's secret back, batched over the dealers
            for _ in range(3):
                idx = rng.sample(range(n), t + 1)
                back = P.shamir_reconstruct(idx, [[want[d][i] for i in idx] for d in range(D)], p)
                assert back == [s % p for s in secrets], (n, D, t, p, idx)


@pytest.mark.parametrize("n,D,t", [(3, 1, 2), (64, 5, 63), (100, 130, 50), (1000, 1, 999)])
def test_explicit_coefficients_all_p_minus_1(n, D, t):
    """the largest carries: every coefficient p - 1, also passed as an unreduced word (2p - 1 means p - 1)"""
    prm = params(n)
    rng = random.Random(n)
    for p in (next_prime(n), P62):
        secrets = secrets_for(D, p, rng)
        coeffs = [[p - 1] * t for _ in range(D)]
        want = restated_shares(n, secrets, t, p, coeffs=coeffs)
        assert P.shamir_shares(prm, secrets, t, p, coeffs=coeffs, host=True).tolist() == want
        wide = [[2 * p - 1] * t for _ in range(D)]
        assert P.shamir_shares(prm, secrets, t, p, coeffs=wide, host=True).tolist() == want
        idx = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct(idx, [[want[d][i] for i in idx] for d in range(D)], p) == [s % p for s in secrets]


def test_degree_zero_copies_the_secret_and_draws_nothing():
    prm = params(64)
    got = P.shamir_shares(prm, [U64, 5], 0, P61, host=True)            # no seeds, no coefficients
    assert got.tolist() == [[U64 % P61] * 64, [5] * 64]


def _host_rc(prm, secrets, D, t, p, seeds, coeffs, out):
    lib = _ffi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return lib.pvw_shamir_shares_host(prm._h, ptr(secrets), D, t, p, ptr(seeds), ptr(coeffs), ptr(out))


def test_rejections():
    n = 64
    prm = params(n)
    se = np.arange(4, dtype=np.uint64)
    sd = np.zeros(4 * 32, dtype=np.uint8)
    out = np.full((4, n), 77, dtype=np.uint64)
    bad_p = [561, 3215031751, 3825123056546413051,         # Carmichael; strong pseudoprime to 2, 3, 5, 7; ... to every prime base <= 23
             65536, 65537 * 65537, n, 61, 2, 1, 0,          # even, a square, p <= n
             1 << 62, next_prime(1 << 62), U64]             # p >= 2^62
    for p in bad_p:
        assert _host_rc(prm, se, 4, 2, p, sd, None, out) == INVALID_PARAMETERS, p
    assert _host_rc(prm, se, 4, n, P61, sd, None, out) == INVALID_PARAMETERS       # degree >= n
    assert _host_rc(prm, se, 0, 2, P61, sd, None, out) == INVALID_PARAMETERS       # D = 0
    assert _host_rc(prm, None, 4, 2, P61, sd, None, out) == INVALID_PARAMETERS     # NULL arguments
    assert _host_rc(prm, se, 4, 2, P61, sd, None, None) == INVALID_PARAMETERS
    assert _host_rc(prm, se, 4, 2, P61, None, None, out) == INVALID_PARAMETERS     # neither seeds nor coefficients
    assert _ffi.lib().pvw_shamir_shares_host(None, se.ctypes.data_as(C.c_void_p), 4, 2, P61, sd.ctypes.data_as(C.c_void_p), None,
                                             out.ctypes.data_as(C.c_void_p)) == INVALID_PARAMETERS
    assert (out == 77).all(), "a refused call writes nothing"
    assert _host_rc(prm, se, 4, n - 1, next_prime(n), sd, None, out) == 0
    # the device entry points refuse the same arguments before any device work (no GPU is needed to be refused)
    for name in ("pvw_shamir_shares", "pvw_shamir_shares_device"):
        for p in (561, 3215031751, 3825123056546413051, n, 1 << 62):
            with pytest.raises(P.PvwError) as e:
                prm._call(name, se.ctypes.data_as(C.c_void_p), 4, 2, p, sd.ctypes.data_as(C.c_void_p), None,
                          out.ctypes.data_as(C.c_void_p), *([None] if name.endswith("device") else []))
            assert e.value.code == INVALID_PARAMETERS, (name, p)


def test_reconstruct_rejections_and_batches():
    p = P61
    rng = random.Random(5)
    # a batch of secrets under one set of weights, against Lagrange interpolation in Python integers
    idx = [0, 7, 3, 999, 12]
    polys = [[rng.randrange(p) for _ in range(5)] for _ in range(9)]
    shares = [[sum(a[j] * pow(i + 1, j, p) for j in range(5)) % p for i in idx] for a in polys]
    assert P.shamir_reconstruct(idx, shares, p) == [a[0] for a in polys]
    assert P.shamir_reconstruct(idx, [[s + p for s in row] for row in shares], p) == [a[0] for a in polys]   # unreduced words
    assert P.shamir_reconstruct(idx, shares[0], p) == polys[0][0]
    lib = _ffi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sh = np.array(shares[0], dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint64)

    def rc(indices, modulus=p, count=None):
        ix = np.array(indices, dtype=np.uint64)
        return lib.pvw_shamir_reconstruct(modulus, ptr(ix), ptr(sh), len(ix) if count is None else count, 1, ptr(out))
    assert rc(idx) == 0
    assert rc(idx, count=0) == INVALID_PARAMETERS
    assert rc([0, 7, 3, 7, 12]) == INVALID_PARAMETERS                  # duplicate
    assert rc([0, 1, 2, 3, 65536], modulus=65537) == INVALID_PARAMETERS   # index >= p - 1: the point would be 0 mod p
    assert rc([0, 1, 2, 3, 65535], modulus=65537) == 0
    assert rc([0, 1, 2, 3, U64]) == INVALID_PARAMETERS
    for bad in (561, 3215031751, 3825123056546413051, 1 << 62, 0, 1):
        assert rc(idx, modulus=bad) == INVALID_PARAMETERS, bad
    assert lib.pvw_shamir_reconstruct(p, None, ptr(sh), 5, 1, ptr(out)) == INVALID_PARAMETERS
    assert lib.pvw_shamir_reconstruct(p, ptr(np.array(idx, dtype=np.uint64)), None, 5, 1, ptr(out)) == INVALID_PARAMETERS
    assert lib.pvw_shamir_reconstruct(p, ptr(np.array(idx, dtype=np.uint64)), ptr(sh), 5, 1, None) == INVALID_PARAMETERS


def test_deal_argument_errors_come_before_the_device():
    """the encrypt-multi checks first (here: no public key loaded), whatever the Shamir arguments are"""
    prm = params(8)
    se = np.arange(3, dtype=np.uint64)
    sd = np.zeros(3 * 32, dtype=np.uint8)
    c1 = np.zeros((3, prm.k, prm.L, prm.l), dtype=np.uint64)
    c2 = np.zeros((3, prm.n, prm.L, prm.l), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    with pytest.raises(P.PvwError) as e:
        prm._call("pvw_deal_shares", ptr(se), 3, 2, 561, ptr(sd), ptr(c1), ptr(c2), P.REPR_NTT)
    assert e.value.code == INVALID_PARAMETERS and "public key" in str(e.value)
    with pytest.raises(P.PvwError) as e:
        prm._call("pvw_deal_shares", ptr(se), 0, 2, P61, ptr(sd), ptr(c1), ptr(c2), P.REPR_NTT)
    assert e.value.code == INVALID_PARAMETERS
    with pytest.raises(P.PvwError) as e:
        prm._call("pvw_deal_shares", None, 3, 2, P61, ptr(sd), ptr(c1), ptr(c2), P.REPR_NTT)
    assert e.value.code == INVALID_PARAMETERS


# ---- C++ mirror -------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "shamir.cpp")
EXE = os.path.join(ROOT, "build", "shamir_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_shares_and_reconstructs_on_the_host():
    """pvw_host::shamir_shares(host = true) and shamir_reconstruct need no GPU: the program's host half runs everywhere"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

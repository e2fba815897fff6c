"""Packed Shamir sharing on the host side: pvw_shamir_shares_packed_host against a restatement of the contract in
Python integers (f_d built from the definition with pow(., -1, p), coefficients from test_shamir_host.restated_coeffs), pack = 1
against pvw_shamir_shares_host word for word, pvw_shamir_reconstruct_packed and the corrected reconstruction giving every
secret back, the argument errors, and the mirrors.  No device compute here; the kernels and the fused deal are checked in
tests/test_gpu_shamir_packed.py.

The grid.  Shapes (n, D, K, t) are the ones the GPU test runs (fewer terms than waves, the secret/random boundary on and off
a wave edge, D beyond one launch, several chunks per wave); p in {smallest prime >= n + K, 65537, the prime above 2^31,
2^61 - 1, the largest prime below 2^62} at every shape; secrets start with 2^64 - 1, 0, p, p - 1."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from test_shamir_host import CASES, P31, P61, P62, U64, INVALID_PARAMETERS, next_prime, params, restated_coeffs, seeds_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pvw_shamir_shares_packed_host", "pvw_shamir_shares_packed_device", "pvw_shamir_shares_packed", "pvw_deal_shares_packed",
       "pvw_deal_shares_packed_device", "pvw_deal_shares_packed_rs", "pvw_deal_shares_packed_rs_device",
       "pvw_shamir_reconstruct_packed"]


def first_prime_from(x):
    return x if M.is_prime(x) else next_prime(x)


def primes_for(n, K):
    return sorted({first_prime_from(n + K), 65537, P31, P61, P62})


def packed_secrets(D, K, p, rng):
    """[D][K] unreduced words: the extremes first, then any 64-bit word"""
    fixed = [U64, 0, p, p - 1, U64 - 1, 1 << 63]
    flat = [fixed[e] if e < len(fixed) else rng.getrandbits(64) for e in range(D * K)]
    return [flat[d * K:(d + 1) * K] for d in range(D)]


def basis(n, K, p):
    """(L, Z): L[j][i] = L_j(i + 1), the Lagrange basis polynomial of -j among 0, -1, ..., -(K-1); Z[i] = prod_m (i + 1 + m)"""
    Z = []
    for i in range(n):
        z = 1
        for m in range(K):
            z = z * (i + 1 + m) % p
        Z.append(z)
    inv = [0] + [pow(v, -1, p) for v in range(1, n + K)]       # of every x + m
    L = []
    for j in range(K):
        den = 1
        for m in range(K):
            if m != j:
                den = den * ((-j) - (-m)) % p
        dinv = pow(den, -1, p)
        L.append([Z[i] * inv[i + 1 + j] % p * dinv % p for i in range(n)])   # prod_{m != j}(x + m) / prod_{m != j}(m - j)
    return L, Z


@functools.lru_cache(maxsize=None)
def drawn_coeffs(seed, t, p):
    return restated_coeffs(seed, t, p)


def restated_packed(n, secrets, K, t, p, seeds=None, coeffs=None):
    L, Z = basis(n, K, p)
    rows = []
    for d, s in enumerate(secrets):
        a = [c % p for c in coeffs[d]] if coeffs is not None else drawn_coeffs(seeds[d], t, p)
        row = []
        for i in range(n):
            x = i + 1
            r = 0                                          # a_1 + a_2 x + ... + a_t x^(t-1)
            for c in reversed(a):
                r = (r * x + c) % p
            row.append((sum((s[j] % p) * L[j][i] for j in range(K)) + Z[i] * r) % p)
        rows.append(row)
    return rows


# (n, D, [(K, t)]): the shapes of tests/test_gpu_shamir_packed.py
SHAPES = [
    (3, 1, [(1, 2), (2, 1), (3, 0)]),
    (3, 5, [(1, 2), (2, 1), (3, 0)]),
    (64, 5, [(1, 63), (64, 0), (32, 32), (33, 31), (5, 2)]),
    (100, 130, [(3, 50), (50, 50)]),
    (300, 5, [(130, 140), (256, 1), (1, 299)]),
    (1000, 1, [(500, 500)]),
]


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_host_shares_equal_the_definition_and_reconstruct(shape):
    n, D, kts = SHAPES[shape]
    prm = params(n)
    rng = random.Random(2000 + shape)
    for K, t in kts:
        for p in primes_for(n, K):
            secrets = packed_secrets(D, K, p, rng)
            seeds = seeds_for(D, tag=t)
            want = restated_packed(n, secrets, K, t, p, seeds=seeds)
            got = P.shamir_shares_packed(prm, secrets, t, p, seeds=seeds if t else None, host=True)
            assert got.tolist() == want, (n, D, K, t, p)
            # the polynomial passes through the secrets: random subsets of t + K parties give every secret back
            for _ in range(2):
                idx = rng.sample(range(n), t + K)
                back = P.shamir_reconstruct_packed(idx, [[want[d][i] for i in idx] for d in range(D)], p, K)
                assert back == [[s % p for s in row] for row in secrets], (n, D, K, t, p, idx)
            # ... and they predict every other share (deg f <= t + K - 1): the plain reconstruction's weights at another point
            if t + K < n:
                idx = rng.sample(range(n), t + K)
                extra = next(i for i in range(n) if i not in idx)
                xs = [i + 1 for i in idx]
                ws = []
                for a, xa in enumerate(xs):
                    num = den = 1
                    for b, xb in enumerate(xs):
                        if a != b:
                            num, den = num * (extra + 1 - xb) % p, den * (xa - xb) % p
                    ws.append(num * pow(den, -1, p) % p)
                for d in (0, D - 1):
                    assert sum(want[d][i] * w for i, w in zip(idx, ws)) % p == want[d][extra], (n, K, t, p, d)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_pack_1_equals_the_unpacked_call_word_for_word(case):
    n, D, degrees, primes = CASES[case]
    prm = params(n)
    rng = random.Random(3000 + case)
    for p in primes:
        for t in degrees:
            secrets = [rng.getrandbits(64) for _ in range(D)]
            secrets[0] = U64
            seeds = seeds_for(D, tag=t)
            old = P.shamir_shares(prm, secrets, t, p, seeds=seeds, host=True)
            new = P.shamir_shares_packed(prm, [[s] for s in secrets], t, p, seeds=seeds, host=True)
            assert np.array_equal(old, new), (n, D, t, p)
            if t:
                coeffs = [[rng.getrandbits(64) for _ in range(t)] for _ in range(D)]
                old = P.shamir_shares(prm, secrets, t, p, coeffs=coeffs, host=True)
                new = P.shamir_shares_packed(prm, [[s] for s in secrets], t, p, coeffs=coeffs, host=True)
                assert np.array_equal(old, new), (n, D, t, p, "coeffs")


@pytest.mark.parametrize("n,D,K,t", [(3, 5, 2, 1), (64, 5, 33, 31), (100, 7, 50, 50), (300, 2, 256, 1)])
def test_zero_coefficients_interpolate_the_secrets(n, D, K, t):
    """explicit all-zero coefficients leave the polynomial of degree <= K - 1 through the secrets: Lagrange interpolation in
    Python integers over the points 0, -1, ..., -(K-1), evaluated at the parties' points"""
    prm = params(n)
    rng = random.Random(n + K)
    for p in (first_prime_from(n + K), P61):
        secrets = packed_secrets(D, K, p, rng)
        got = P.shamir_shares_packed(prm, secrets, t, p, coeffs=[[0] * t for _ in range(D)], host=True).tolist()
        L, _ = basis(n, K, p)
        assert got == [[sum((s[j] % p) * L[j][i] for j in range(K)) % p for i in range(n)] for s in secrets]
        back = P.shamir_reconstruct_packed(list(range(K)), [row[:K] for row in got], p, K)      # K shares are enough
        assert back == [[v % p for v in s] for s in secrets]
        if K == 1:
            assert got == [[s[0] % p] * n for s in secrets]


def _corrupt(rows, p, count, rng, wrong):
    """`wrong` columns of every row (its own random choice) replaced by another residue"""
    out, where = [], []
    for row in rows:
        row = list(row)
        cols = sorted(rng.sample(range(count), wrong))
        for c in cols:
            row[c] = (row[c] + 1 + rng.randrange(p - 1)) % p
        out.append(row)
        where.append(cols)
    return out, where


@pytest.mark.parametrize("n,D,K,t", [(12, 4, 3, 4), (64, 5, 5, 2), (64, 3, 33, 20), (100, 3, 3, 50), (12, 4, 1, 4), (64, 5, 1, 31)])
def test_corrected_reconstruction_and_degree_check(n, D, K, t):
    p = P61            # large enough that one wrong share too many stays undecodable (a mis-decode needs a chance hit in Z_p)
    prm = params(n)
    rng = random.Random(n * K + t)
    secrets = packed_secrets(D, K, p, rng)
    shares = P.shamir_shares_packed(prm, secrets, t, p, seeds=seeds_for(D, tag=9), host=True).tolist()
    want = [[v % p for v in s] for s in secrets]
    idx = list(range(n))
    rng.shuffle(idx)
    rows = [[shares[d][i] for i in idx] for d in range(D)]
    # the sharing has degree t + K - 1: the checked reconstruction finds no column off the basis polynomial
    _, bad, col_bad = P.shamir_reconstruct_checked(None, idx, rows, t + K - 1, p, host=True)
    assert not bad.any() and not col_bad.any()
    E = (n - t - K) // 2
    noisy, where = _corrupt(rows, p, n, rng, E)
    got, nerr, col_err, mask = P.shamir_reconstruct_packed_corrected(None, idx, noisy, t, p, K, host=True)
    assert got == want
    assert nerr.tolist() == [E] * D and int(col_err.sum()) == E * D
    if K == 1:                                                  # an ordinary sharing: the report of shamir_reconstruct_corrected
        ref = P.shamir_reconstruct_corrected(None, idx, noisy, t, p, host=True)
        assert [r[0] for r in got] == ref[0] and all(np.array_equal(a, b) for a, b in zip((nerr, col_err, mask), ref[1:]))
    for d in range(D):
        assert [c for c in range(n) if (int(mask[d][c // 64]) >> (c % 64)) & 1] == where[d]
    # party-major input (what decrypt_all_party_sums returns) is the same call
    got_pm = P.shamir_reconstruct_packed_corrected(None, idx, np.array(noisy, dtype=np.uint64).T.tolist(), t, p, K, host=True,
                                                   layout="party_major")[0]
    assert got_pm == want
    # one more wrong share than can be corrected: the row is reported, and all 0
    worse, _ = _corrupt(rows, p, n, rng, E + 1)
    got, nerr, _, mask = P.shamir_reconstruct_packed_corrected(None, idx, worse, t, p, K, host=True)
    assert nerr.tolist() == [P.SHAMIR_UNDECODABLE] * D
    assert got == [[0] * K for _ in range(D)] and not mask.any()
    assert P.shamir_packed_secret_indices(p, K) == [p - 1 - j for j in range(1, K)]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _host_rc(prm, secrets, D, K, t, p, seeds, coeffs, out):
    return _ffi.lib().pvw_shamir_shares_packed_host(prm._h, _ptr(secrets), D, K, t, p, _ptr(seeds), _ptr(coeffs), _ptr(out))


def test_rejections():
    n, K = 64, 4
    prm = params(n)
    se = np.arange(4 * K, dtype=np.uint64)
    sd = np.zeros(4 * 32, dtype=np.uint8)
    out = np.full((4, n), 77, dtype=np.uint64)
    bad_p = [561, 3215031751, 3825123056546413051, 65536, 65537 * 65537, n + K - 1, n, 61, 2, 1, 0,
             1 << 62, next_prime(1 << 62), U64]
    for p in bad_p:
        assert _host_rc(prm, se, 4, K, 2, p, sd, None, out) == INVALID_PARAMETERS, p
    assert _host_rc(prm, se, 4, 0, 2, P61, sd, None, out) == INVALID_PARAMETERS           # pack = 0
    assert _host_rc(prm, se, 4, K, n - K + 1, P61, sd, None, out) == INVALID_PARAMETERS   # degree + pack > n
    assert _host_rc(prm, se, 4, n + 1, 0, P61, sd, None, out) == INVALID_PARAMETERS
    assert _host_rc(prm, se, 4, U64 & 0xFFFFFFFF, 2, P61, sd, None, out) == INVALID_PARAMETERS
    assert _host_rc(prm, se, 0, K, 2, P61, sd, None, out) == INVALID_PARAMETERS           # D = 0
    assert _host_rc(prm, None, 4, K, 2, P61, sd, None, out) == INVALID_PARAMETERS         # NULL arguments
    assert _host_rc(prm, se, 4, K, 2, P61, sd, None, None) == INVALID_PARAMETERS
    assert _host_rc(prm, se, 4, K, 2, P61, None, None, out) == INVALID_PARAMETERS         # neither seeds nor coefficients
    assert _ffi.lib().pvw_shamir_shares_packed_host(None, _ptr(se), 4, K, 2, P61, _ptr(sd), None, _ptr(out)) == INVALID_PARAMETERS
    assert (out == 77).all(), "a refused call writes nothing"
    # the edge of p >= n + pack: 67 = n + 3 is prime, so pack = 3 is accepted there and pack = 4 (p = n + pack - 1) is not
    assert M.is_prime(67)
    assert _host_rc(prm, se, 4, 3, 2, 67, sd, None, out) == 0
    assert _host_rc(prm, se, 4, 4, 2, 67, sd, None, out) == INVALID_PARAMETERS
    assert _host_rc(prm, se, 4, K, n - K, first_prime_from(n + K), sd, None, out) == 0    # degree + pack = n, the smallest prime
    assert _host_rc(prm, se, 4, K, 0, P61, None, None, out) == 0                          # degree 0 needs no seeds
    # the device entry points refuse the same arguments before any device work (no GPU is needed to be refused)
    for name in ("pvw_shamir_shares_packed", "pvw_shamir_shares_packed_device"):
        tail = [None] if name.endswith("device") else []
        for pack, t, p in [(K, 2, 561), (K, 2, n + K - 1), (K, 2, 1 << 62), (0, 2, P61), (K, n - K + 1, P61)]:
            with pytest.raises(P.PvwError) as e:
                prm._call(name, _ptr(se), 4, pack, t, p, _ptr(sd), None, _ptr(out), *tail)
            assert e.value.code == INVALID_PARAMETERS, (name, pack, t, p)
        with pytest.raises(P.PvwError) as e:
            prm._call(name, _ptr(se), 0, K, 2, P61, _ptr(sd), None, _ptr(out), *tail)
        assert e.value.code == INVALID_PARAMETERS


def test_reconstruct_packed_rejections():
    p, K = 65537, 3
    lib = _ffi.lib()
    sh = np.arange(5, dtype=np.uint64)
    out = np.zeros(K, dtype=np.uint64)

    def rc(indices, modulus=p, pack=K, count=None):
        ix = np.array(indices, dtype=np.uint64)
        return lib.pvw_shamir_reconstruct_packed(modulus, pack, _ptr(ix), _ptr(sh), len(ix) if count is None else count, 1, _ptr(out))
    idx = [0, 7, 3, 999, 12]
    assert rc(idx) == 0
    assert rc(idx, pack=0) == INVALID_PARAMETERS
    assert rc(idx, count=0) == INVALID_PARAMETERS
    assert rc([0, 7, 3, 7, 12]) == INVALID_PARAMETERS                  # duplicate
    assert rc([0, 1, 2, 3, p - K]) == INVALID_PARAMETERS               # index p - pack: the point p - K + 1 is secret K - 1's
    assert rc([0, 1, 2, 3, p - K - 1]) == 0
    assert rc([0, 1, 2, 3, p - 2], pack=1) == 0                        # pack = 1: the rule of pvw_shamir_reconstruct
    assert rc([0, 1, 2, 3, p - 1], pack=1) == INVALID_PARAMETERS
    assert rc([0, 1, 2, 3, U64]) == INVALID_PARAMETERS
    for bad in (561, 3215031751, 3825123056546413051, 1 << 62, 0, 1):
        assert rc(idx, modulus=bad) == INVALID_PARAMETERS, bad
    ix = np.array(idx, dtype=np.uint64)
    assert lib.pvw_shamir_reconstruct_packed(p, K, None, _ptr(sh), 5, 1, _ptr(out)) == INVALID_PARAMETERS
    assert lib.pvw_shamir_reconstruct_packed(p, K, _ptr(ix), None, 5, 1, _ptr(out)) == INVALID_PARAMETERS
    assert lib.pvw_shamir_reconstruct_packed(p, K, _ptr(ix), _ptr(sh), 5, 1, None) == INVALID_PARAMETERS
    # pack = 1 is pvw_shamir_reconstruct
    rng = random.Random(11)
    rows = [[rng.getrandbits(64) for _ in idx] for _ in range(4)]
    assert [r[0] for r in P.shamir_reconstruct_packed(idx, rows, P61, 1)] == P.shamir_reconstruct(idx, rows, P61)


def test_deal_argument_errors_come_before_the_device():
    """the encrypt-multi checks first (here: no public key loaded), whatever the Shamir arguments are; then the packed ones"""
    prm = params(8)
    K = 2
    se = np.arange(3 * K, dtype=np.uint64)
    sd = np.zeros(3 * 32, dtype=np.uint8)
    c1 = np.zeros((3, prm.k, prm.L, prm.l), dtype=np.uint64)
    c2 = np.zeros((3, prm.n, prm.L, prm.l), dtype=np.uint64)
    with pytest.raises(P.PvwError) as e:
        prm._call("pvw_deal_shares_packed", _ptr(se), 3, 0, 2, 561, _ptr(sd), _ptr(c1), _ptr(c2), P.REPR_NTT)
    assert e.value.code == INVALID_PARAMETERS and "public key" in str(e.value)
    for name, tail in (("pvw_deal_shares_packed", []), ("pvw_deal_shares_packed_device", [None])):
        with pytest.raises(P.PvwError) as e:
            prm._call(name, _ptr(se), 0, K, 2, P61, _ptr(sd), _ptr(c1), _ptr(c2), P.REPR_NTT, *tail)
        assert e.value.code == INVALID_PARAMETERS
        with pytest.raises(P.PvwError) as e:
            prm._call(name, None, 3, K, 2, P61, _ptr(sd), _ptr(c1), _ptr(c2), P.REPR_NTT, *tail)
        assert e.value.code == INVALID_PARAMETERS
    with pytest.raises(P.PvwError):
        P.shamir_shares_packed(prm, [[1, 2], [3]], 1, P61, seeds=seeds_for(2), host=True)      # ragged secrets


# ---- C++ mirror -------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "shamir_packed.cpp")
EXE = os.path.join(ROOT, "build", "shamir_packed_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_shares_and_reconstructs_on_the_host():
    """the mirror compiles against the header, and its host half (restatement, both reconstructions) needs no GPU"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

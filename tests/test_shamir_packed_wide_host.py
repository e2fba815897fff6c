"""Packed Shamir dealing over a prime field of up to 256 bits, the CPU half: pvw_shamir_shares_packed_wide_host
against the definition in Python's own integers (explicit coefficients, and drawn ones with the draw rule restated on the model's
ChaCha8), pack = 1 against pvw_shamir_shares_wide_host, pvw_shamir_reconstruct_packed_wide, the corrected way back on the host
restatements, every refusal, the kernels' sequence as a stand-alone program under sanitizers, the names and the C++ mirror.  No
device is used."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from test_shamir_wide_host import CSRC, LIBDIR, PRIMES, ROOT, SECP_N, W256, edge_values, evaluate, ints, params, restated_coeffs, seeds_for

NEW = ["pvw_shamir_shares_packed_wide_host", "pvw_shamir_shares_packed_wide_device", "pvw_shamir_shares_packed_wide",
       "pvw_deal_shares_packed_wide", "pvw_deal_shares_packed_wide_device", "pvw_deal_shares_packed_wide_rs",
       "pvw_deal_shares_packed_wide_rs_device", "pvw_shamir_reconstruct_packed_wide"]
MIRRORS = ["shamir_shares_packed_wide", "deal_party_shares_packed_wide", "shamir_reconstruct_packed_wide",
           "shamir_reconstruct_packed_wide_corrected"]


def packed_evaluate(secrets, coeffs, n, p):
    """f(i + 1) for i < n, f = sum_j s_j L_j + Z (a_1 + a_2 x + ...), L_j the basis of -j among 0, -1, .., -(K-1)"""
    K = len(secrets)
    out = []
    for i in range(n):
        x = i + 1
        acc = 0
        for j in range(K):
            num = den = 1
            for m in range(K):
                if m != j:
                    num = num * (x + m) % p
                    den = den * (m - j) % p                       # (-j) - (-m)
            acc += secrets[j] * num * pow(den, -1, p)
        z = 1
        for m in range(K):
            z = z * (x + m) % p
        out.append((acc + z * sum(c * pow(x, e, p) for e, c in enumerate(coeffs))) % p)
    return out


def test_exports_of_both_libraries_and_the_header():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    assert "#define PVW_WIDE_MAX_PACK 1024" in header
    for name in NEW:
        assert name in _ffi._SIGNATURES and ("PVW_API int32_t " + name + "(") in header, name
        for lib in ("libpvw_hip.so", "libpvw_hip_tuning.so"):
            assert hasattr(C.CDLL(os.path.join(LIBDIR, lib)), name), (lib, name)
    for name in MIRRORS:
        assert name in P.__all__ and callable(getattr(P, name)), name
    hpp = open(os.path.join(ROOT, "pvw_rs_amd", "host", "pvw.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "pvw", "src", "crypto.rs")).read()
    for name in MIRRORS:
        assert ("inline" in hpp and name + "(" in hpp) and "pub fn " + name in rs, name


@pytest.mark.parametrize("p", PRIMES, ids=lambda p: f"{p.bit_length()}bit")
def test_host_shares_equal_the_definition_in_big_integers(p):
    assert len(PRIMES) == 13
    rng = random.Random(p & 0xFFFF)
    n, D = 9, 5
    pr = params(n)
    for K, t in ((1, 3), (2, 0), (3, 2), (4, 5), (9, 0), (5, 4)):
        assert p >= n + K
        secrets = [[edge_values(p, rng, 4)[(d + j) % 4] if d < 4 else rng.getrandbits(256) for j in range(K)] for d in range(D)]
        coeffs = [[edge_values(p, rng, 4)[(d + j + 1) % 4] if d < 4 else rng.getrandbits(256) for j in range(t)] for d in range(D)]
        got = ints(P.shamir_shares_packed_wide(pr, secrets, K, t, p, coeffs=coeffs, host=True))
        assert got == [packed_evaluate(secrets[d], coeffs[d], n, p) for d in range(D)], ("explicit", K, t)
        seeds = seeds_for(D, tag=t)
        got = ints(P.shamir_shares_packed_wide(pr, secrets, K, t, p, seeds=seeds if t else None, host=True))
        assert got == [packed_evaluate(secrets[d], restated_coeffs(seeds[d], t, p), n, p) for d in range(D)], ("drawn", K, t)
        assert all(v < p for row in got for v in row)


@pytest.mark.parametrize("p", PRIMES, ids=lambda p: f"{p.bit_length()}bit")
def test_pack_one_is_the_wide_call(p):
    """the grid of test_host_shares_equal_big_integer_evaluation: n = 9, D = 5, t in (0, 1, n - 1), explicit and drawn"""
    rng = random.Random(p & 0xFFFF)
    n, D = 9, 5
    pr = params(n)
    for t in (0, 1, n - 1):
        secrets = edge_values(p, rng, D)
        coeffs = [[edge_values(p, rng, 4)[(d + j) % 4] if d < 4 else rng.getrandbits(256) for j in range(t)] for d in range(D)]
        want = P.shamir_shares_wide(pr, secrets, t, p, coeffs=coeffs, host=True)
        assert np.array_equal(P.shamir_shares_packed_wide(pr, [[s] for s in secrets], 1, t, p, coeffs=coeffs, host=True), want)
        assert ints(want) == [evaluate(secrets[d], coeffs[d], n, p) for d in range(D)]
        seeds = seeds_for(D, tag=t)
        want = P.shamir_shares_wide(pr, secrets, t, p, seeds=seeds, host=True)
        assert np.array_equal(P.shamir_shares_packed_wide(pr, [[s] for s in secrets], 1, t, p, seeds=seeds, host=True), want)


def test_degree_zero_and_all_zero_coefficients():
    n, K, p = 11, 4, SECP_N
    pr = params(n)
    secrets = [[5, p - 1, W256, 0], [1, 2, 3, 4]]
    zero = P.shamir_shares_packed_wide(pr, secrets, K, 0, p, host=True)              # no seeds, nothing drawn
    assert ints(zero) == [packed_evaluate(s, [], n, p) for s in secrets]
    assert np.array_equal(P.shamir_shares_packed_wide(pr, secrets, K, 3, p, coeffs=[[0, 0, 0], [p, 0, p]], host=True), zero)
    # the polynomial through K points has degree K - 1: K of its shares give the secrets back
    idx = [10, 2, 5, 7]
    assert P.shamir_reconstruct_packed_wide(idx, zero[:, idx, :], p, K) == [[v % p for v in s] for s in secrets]


@pytest.mark.parametrize("p", [65537, 2**64 + 13, 2**89 - 1, SECP_N, 2**256 - 189], ids=lambda p: f"{p.bit_length()}bit")
def test_reconstruction_from_random_subsets_and_prediction(p):
    rng = random.Random(p & 0xFFF)
    n, D, t, K = 17, 3, 5, 4
    pr = params(n)
    secrets = [[rng.getrandbits(256) for _ in range(K)] for _ in range(D)]
    words = P.shamir_shares_packed_wide(pr, secrets, K, t, p, seeds=seeds_for(D), host=True)
    shares = ints(words)
    want = [[v % p for v in row] for row in secrets]
    for _ in range(3):
        idx = rng.sample(range(n), t + K)
        assert P.shamir_reconstruct_packed_wide(idx, [[shares[d][i] for i in idx] for d in range(D)], p, K) == want
        assert P.shamir_reconstruct_packed_wide(idx, words[:, idx, :], p, K) == want
    # prediction of another share: t + K shares fix the polynomial, whose value at any other party the wide evaluate call gives
    idx = rng.sample(range(n), t + K)
    other = [i for i in range(n) if i not in idx][:2]
    values, _, nerr, _, _ = P.shamir_evaluate_wide_corrected(None, idx, words[:, idx, :], t + K - 1, p, other, host=True)
    assert values == [[shares[d][i] for i in other] for d in range(D)] and not nerr.any()
    # fewer than t + K shares do not determine the secrets
    idx = rng.sample(range(n), t + K - 1)
    assert P.shamir_reconstruct_packed_wide(idx, words[:, idx, :], p, K) != want


def test_corrected_way_back_on_the_host_restatements():
    rng = random.Random(11)
    p, n, D, t, K = SECP_N, 14, 3, 3, 3
    pr = params(n)
    secrets = [[rng.randrange(p) for _ in range(K)] for _ in range(D)]
    words = P.shamir_shares_packed_wide(pr, secrets, K, t, p, seeds=seeds_for(D), host=True)
    idx = list(range(n))
    rng.shuffle(idx)
    rows = np.ascontiguousarray(words[:, idx, :])
    sec, nerr, col_err, mask = P.shamir_reconstruct_packed_wide_corrected(None, p, K, t, idx, rows, host=True)
    assert sec == secrets and not nerr.any() and not col_err.any() and not mask.any()
    bent = rows.copy()                                              # E = (14 - 5 - 1) // 2 = 4
    bent[0, 0, 0] ^= np.uint64(1)                                  # inside the columns the corrected shares are taken at
    bent[0, 9, 3] ^= np.uint64(1 << 17)
    for c in (1, 2, 3, 4, 5):
        bent[2, c, 1] ^= np.uint64(4)                              # five errors: beyond E
    sec, nerr, col_err, mask = P.shamir_reconstruct_packed_wide_corrected(None, p, K, t, idx, bent, host=True)
    assert sec[:2] == secrets[:2] and sec[2] == [0] * K
    assert nerr.tolist() == [2, 0, P.SHAMIR_UNDECODABLE] and int(mask[0, 0]) == 1 | (1 << 9) and int(mask[2, 0]) == 0
    erased = np.zeros((D, n), dtype=bool)
    erased[2, 1] = erased[2, 2] = True                             # 2 * 3 + 2 = 8 <= 14 - 5 - 1
    sec, nerr, _, _ = P.shamir_reconstruct_packed_wide_corrected(None, p, K, t, idx, bent, erased, host=True)
    assert sec == secrets and nerr.tolist() == [2, 0, 3]
    # pack = 1 routes to shamir_reconstruct_wide_corrected
    one = P.shamir_shares_wide(pr, [s[0] for s in secrets], t, p, seeds=seeds_for(D), host=True)[:, idx, :]
    sec, nerr, _, _ = P.shamir_reconstruct_packed_wide_corrected(None, p, 1, t, idx, one, host=True)
    assert sec == [[s[0]] for s in secrets] and not nerr.any()


def next_prime(v):
    while True:
        if v % 2 and all(v % q for q in range(3, int(v ** 0.5) + 1, 2)):
            return v
        v += 1


def test_refusals():
    n = 70
    pr = params(n)
    call = lambda K, t, p, **kw: P.shamir_shares_packed_wide(pr, [[1] * K], K, t, p, host=True, **kw)
    # p = n + pack - 1 is refused when prime, the smallest prime >= n + pack is accepted
    for K in (1, 2, 4, 10, 14):
        p = n + K - 1
        if next_prime(p) == p:
            with pytest.raises(P.PvwError) as e:
                call(K, 0, p)
            assert e.value.code == 1, K
        q = next_prime(n + K)
        assert ints(call(K, 0, q))[0] == packed_evaluate([1] * K, [], n, q), K
    assert [K for K in (1, 2, 4, 10, 14) if next_prime(n + K - 1) == n + K - 1] == [2, 4, 10, 14]     # 71, 73, 79, 83
    for K, t, p in ((0, 0, SECP_N), (1025, 0, SECP_N), (3, n - 2, SECP_N), (n, 1, SECP_N), (3, 0, SECP_N - 1), (3, 0, 71)):
        with pytest.raises(P.PvwError) as e:
            P.shamir_shares_packed_wide(pr, [[1] * max(K, 1)] if K else np.zeros((1, 1, 4), dtype=np.uint64), K, t, p, coeffs=[[1] * t],
                                        host=True)
        assert e.value.code == 1, (K, t, p)
    assert ints(call(3, n - 3, SECP_N, coeffs=[[0] * (n - 3)]))[0] == packed_evaluate([1] * 3, [], n, SECP_N)   # degree + pack = n
    with pytest.raises(P.PvwError) as e:                           # pack 1025 where degree + pack <= n: the limit itself
        P.shamir_shares_packed_wide(params(1100), [[1] * 1025], 1025, 0, 2**61 - 1, host=True)
    assert e.value.code == 1 and "PVW_WIDE_MAX_PACK" in str(e.value)
    with pytest.raises(P.PvwError):
        call(3, 2, SECP_N)                                          # neither seeds nor coefficients
    # every entry point refuses before any device work (this machine has no device to reach)
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    pm = api._wide_modulus(SECP_N)
    one = np.ones((4, 4), dtype=np.uint64)
    out = np.zeros((n, 4), dtype=np.uint64)
    sd = np.zeros(32 * 16, dtype=np.uint8)
    for name in ("pvw_shamir_shares_packed_wide_host", "pvw_shamir_shares_packed_wide", "pvw_shamir_shares_packed_wide_device"):
        tail = (None,) if name.endswith("_device") else ()
        for K, t in ((0, 0), (1025, 0), (3, n - 2)):
            assert getattr(lib, name)(pr._h, ptr(one), 1, K, t, ptr(pm), ptr(sd), None, ptr(out), *tail) == 1, (name, K, t)
        assert getattr(lib, name)(pr._h, ptr(one), 1, 2, 0, None, None, None, ptr(out), *tail) == 1
        assert getattr(lib, name)(pr._h, None, 1, 2, 0, ptr(pm), None, None, ptr(out), *tail) == 1
    for name in ("pvw_deal_shares_packed_wide", "pvw_deal_shares_packed_wide_device", "pvw_deal_shares_packed_wide_rs",
                 "pvw_deal_shares_packed_wide_rs_device"):
        tail = (None,) if name.endswith("_device") else ()
        assert getattr(lib, name)(pr._h, None, 1, 2, 0, ptr(pm), 52, ptr(sd), ptr(out), ptr(out), P.REPR_NTT, *tail) == 1, name
        assert getattr(lib, name)(None, ptr(one), 1, 2, 0, ptr(pm), 52, ptr(sd), ptr(out), ptr(out), P.REPR_NTT, *tail) == 1, name


def test_reconstruction_refusals():
    p = 65537
    ok = [[1, 2, 3]]
    assert P.shamir_reconstruct_packed_wide([0, 1, 2], ok, p, 2) == [[0, p - 1]]    # the line f(x) = x at 0 and -1
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_packed_wide([0, 1, 2], ok, p, 0)                        # pack 0
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_packed_wide([0, 1, 1], ok, p, 2)                        # a duplicate index
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_packed_wide([0, 1, p - 2], ok, p, 2)                    # an index of p - pack: its point is -1
    assert len(P.shamir_reconstruct_packed_wide([0, 1, p - 3], ok, p, 2)[0]) == 2    # p - pack - 1 is the last legal index
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_packed_wide([0, 1, 2], ok, p - 1, 2)                    # an even modulus
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_packed_wide([], [[]], p, 2)                             # no shares
    wide = 2**64 + 13                                              # an index of 2^64 - 2 is below p - 1 but not below p - pack for pack 16
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_packed_wide([0, 2**64 - 2], [[1, 2]], wide, 16)
    assert len(P.shamir_reconstruct_packed_wide([0, 2**64 - 2], [[1, 2]], wide, 2)[0]) == 2
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    one = np.ones((2, 4), dtype=np.uint64)
    assert lib.pvw_shamir_reconstruct_packed_wide(None, 1, ptr(one), ptr(one), 1, 1, ptr(one)) == 1
    assert lib.pvw_shamir_reconstruct_packed_wide(ptr(api._wide_modulus(p)), 1, None, ptr(one), 1, 1, ptr(one)) == 1


def test_kernel_sequence_against_the_definition_under_sanitizers():
    """tests/cpp/shamir_packed_wide.cpp: the basis, weights and packed evaluation kernels restated sequentially over pvw_wide.h,
    against the definition computed another way, for each of the 13 primes.  The only sanitizer run: nothing loaded into Python
    is sanitized."""
    exe = os.path.join(ROOT, "build", "shamir_packed_wide")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_packed_wide.cpp"), "-o", exe])
    out = subprocess.run([exe, "60"] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_WIDE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


SRC = os.path.join(ROOT, "tests", "cpp", "shamir_packed_wide_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_packed_wide_cpp")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_on_the_host():
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_WIDE_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

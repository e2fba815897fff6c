"""Shamir shares over a prime field of up to 256 bits, the CPU half: pvw_shamir_shares_wide_host against Python's
own integers (explicit coefficients, and drawn ones with the draw rule restated on the model's ChaCha8); the kernel's Horner step
as a stand-alone program against long division; the limb helpers; reconstruction; the refusals; the names.  No device is used."""
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
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")
W256 = (1 << 256) - 1

BLS_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
PRIMES = [65537, 2**61 - 1, 2**64 + 13, 2**89 - 1, 2**127 - 1, 2**128 + 51, 2**192 + 133,
          2**252 + 27742317777372353535851937790883648493, 2**255 - 19, 2**255 + 95, BLS_R, SECP_N, 2**256 - 189]
COMPOSITE_255 = (2**127 + 29) * (2**127 + 45)        # two 128-bit primes; the product has 255 bits


def params(n):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(TEST_MODULI).build()


def ints(words):
    """uint64 [..., 4] -> nested lists of ints"""
    a = np.asarray(words)
    flat = [sum(int(row[w]) << (64 * w) for w in range(4)) for row in a.reshape(-1, 4)]
    return np.array(flat, dtype=object).reshape(a.shape[:-1]).tolist()


def seeds_for(D, tag=0):
    return [bytes((11 * d + 5 * i + tag) & 0xFF for i in range(32)) for d in range(D)]


def restated_coeffs(seed, degree, p):
    """a_j (j = 1..degree): the first accepted attempt of the stream (seed, (DOM_SHAMIR << 32) | j); an attempt is four
    next_u64() words, word 0 least significant, masked to bitlen(p) bits, accepted when below p"""
    mask = (1 << p.bit_length()) - 1
    out = []
    for j in range(1, degree + 1):
        g = M.ChaChaRng(seed, P.DOM_SHAMIR, j)
        while True:
            v = sum(g.next_u64() << (64 * w) for w in range(4)) & mask
            if v < p:
                break
        out.append(v)
    return out


def evaluate(secret, coeffs, n, p):
    return [(secret + sum(c * pow(i + 1, j + 1, p) for j, c in enumerate(coeffs))) % p for i in range(n)]


def edge_values(p, rng, count):
    fixed = [0, p - 1, p, W256]
    return [fixed[i] if i < len(fixed) else rng.getrandbits(256) for i in range(count)]


@pytest.mark.parametrize("p", PRIMES, ids=lambda p: f"{p.bit_length()}bit")
def test_host_shares_equal_big_integer_evaluation(p):
    rng = random.Random(p & 0xFFFF)
    n, D = 9, 5
    pr = params(n)
    for t in (0, 1, n - 1):
        secrets = edge_values(p, rng, D)
        coeffs = [[edge_values(p, rng, 4)[(d + j) % 4] if d < 4 else rng.getrandbits(256) for j in range(t)] for d in range(D)]
        got = ints(P.shamir_shares_wide(pr, secrets, t, p, coeffs=coeffs, host=True))
        assert got == [evaluate(secrets[d], coeffs[d], n, p) for d in range(D)], ("explicit", t)
        seeds = seeds_for(D, tag=t)
        got = ints(P.shamir_shares_wide(pr, secrets, t, p, seeds=seeds, host=True))
        assert got == [evaluate(secrets[d], restated_coeffs(seeds[d], t, p), n, p) for d in range(D)], ("drawn", t)


def test_step_function_against_long_division_under_sanitizers():
    """tests/cpp/shamir_wide.cpp: 10^5 seeded cases per prime, x in {1, 2, 2^16, 2^32 - 1, random}, acc and add in {0, p - 1,
    random}, compared with schoolbook long division on unsigned __int128; the word reduction rides along"""
    exe = os.path.join(ROOT, "build", "shamir_wide")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide.cpp"), "-o", exe])
    out = subprocess.run([exe, "100000"] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_limb_helpers_round_trip_and_fold_sums():
    rng = random.Random(7)
    for p, limb_bits in ((65537, 16), (2**61 - 1, 16), (2**61 - 1, 62), (SECP_N, 52), (SECP_N, 62), (2**255 - 19, 52), (2**256 - 189, 16)):
        nl = P.shamir_wide_limbs(p, limb_bits)
        assert nl == -(-p.bit_length() // limb_bits)
        values = [0, p - 1] + [rng.randrange(p) for _ in range(6)]
        limbs = P.shamir_wide_to_limbs(values, limb_bits, nl)
        assert limbs.shape == (nl, len(values))
        assert [[int(limbs[w][i]) for i in range(len(values))] for w in range(nl)] == \
            [[(v >> (w * limb_bits)) & ((1 << limb_bits) - 1) for v in values] for w in range(nl)]
        assert P.shamir_wide_to_limbs(values, limb_bits, plain_modulus=p).tolist() == limbs.tolist()
        assert P.shamir_wide_from_limbs(limbs, p, limb_bits) == values
        # sums of limbs: any 64-bit word, 2^64 - 1 included
        sums = [[(1 << 64) - 1 if (w + i) % 3 == 0 else rng.getrandbits(64) for i in range(5)] for w in range(nl)]
        assert P.shamir_wide_from_limbs(sums, p, limb_bits) == \
            [sum(sums[w][i] << (w * limb_bits) for w in range(nl)) % p for i in range(5)]
    with pytest.raises(P.PvwError):
        P.shamir_wide_to_limbs([1 << 200], 52, 3)                 # does not fit three limbs


def test_limbwise_sums_of_2048_dealers_stay_below_2_63():
    assert 2048 * ((1 << 52) - 1) < 1 << 63 and P.shamir_wide_limbs(2**256 - 189) == 5


@pytest.mark.parametrize("p", [65537, 2**89 - 1, BLS_R, SECP_N, 2**256 - 189], ids=lambda p: f"{p.bit_length()}bit")
def test_reconstruction_from_random_subsets(p):
    rng = random.Random(p & 0xFFF)
    n, D, t = 13, 3, 6
    pr = params(n)
    secrets = [rng.getrandbits(256) for _ in range(D)]
    shares = ints(P.shamir_shares_wide(pr, secrets, t, p, seeds=seeds_for(D), host=True))
    for _ in range(3):
        idx = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct_wide(idx, [[shares[d][i] for i in idx] for d in range(D)], p) == [s % p for s in secrets]
    idx = rng.sample(range(n), t + 1)
    assert P.shamir_reconstruct_wide(idx, [shares[0][i] for i in idx], p) == secrets[0] % p
    words = P.shamir_shares_wide(pr, secrets, t, p, seeds=seeds_for(D), host=True)[:, idx, :]
    assert P.shamir_reconstruct_wide(idx, words, p) == [s % p for s in secrets]
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide([1, 1], [5, 5], p)              # a duplicate index
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide([0, 65536], [5, 5], 65537)      # an index of p - 1: its point is 0


def test_refusals():
    n = 7
    pr = params(n)
    ok = dict(coeffs=[[1, 2]], host=True)
    assert ints(P.shamir_shares_wide(pr, [3], 2, SECP_N, **ok))[0] == evaluate(3, [1, 2], n, SECP_N)
    for bad in (COMPOSITE_255, SECP_N - 1, 2**256 - 190, 7, 5, 4, 1, 0, 561, 3 * (2**89 - 1)):
        with pytest.raises(P.PvwError) as e:
            P.shamir_shares_wide(pr, [3], 2, bad, **ok)
        assert e.value.code == 1, bad
    assert COMPOSITE_255.bit_length() == 255
    with pytest.raises(P.PvwError):
        P.shamir_shares_wide(pr, [3], n, SECP_N, coeffs=[[1] * n], host=True)      # degree >= n
    with pytest.raises(P.PvwError):
        P.shamir_shares_wide(pr, [], 0, SECP_N, host=True)                         # no dealers
    with pytest.raises(P.PvwError):
        P.shamir_shares_wide(pr, [3], 2, SECP_N, host=True)                        # neither seeds nor coefficients
    with pytest.raises(P.PvwError):
        P.shamir_wide_limbs(SECP_N, 15)
    with pytest.raises(P.PvwError):
        P.shamir_wide_limbs(SECP_N, 63)
    assert P.shamir_wide_limbs(SECP_N, 16) == 16
    with pytest.raises(P.PvwError):
        P.shamir_wide_limbs(SECP_N - 1, 52)                                        # even
    # NL > 16: 256 bits in limbs of 16 bits are exactly 16 and narrower limbs are refused, so the limit binds where the caller
    # states the count
    with pytest.raises(P.PvwError):
        P.shamir_wide_to_limbs([1], 16, 17)
    with pytest.raises(P.PvwError):
        P.shamir_wide_from_limbs([[1]] * 17, SECP_N, 16)
    with pytest.raises(P.PvwError):
        P.shamir_wide_from_limbs([[1]], COMPOSITE_255, 52)
    # NULL arguments, straight at the C ABI
    import ctypes as C
    lib = _ffi.lib()
    pm = np.array([(SECP_N >> (64 * w)) & (2**64 - 1) for w in range(4)], dtype=np.uint64)
    one = np.zeros(4, dtype=np.uint64)
    out = np.zeros((n, 4), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    nl = C.c_uint32()
    assert lib.pvw_shamir_wide_limbs(None, 52, C.byref(nl)) == 1 and lib.pvw_shamir_wide_limbs(ptr(pm), 52, None) == 1
    assert lib.pvw_shamir_shares_wide_host(pr._h, ptr(one), 1, 0, None, None, None, ptr(out)) == 1
    assert lib.pvw_shamir_shares_wide_host(pr._h, None, 1, 0, ptr(pm), None, None, ptr(out)) == 1
    assert lib.pvw_shamir_shares_wide_host(pr._h, ptr(one), 1, 0, ptr(pm), None, None, None) == 1
    assert lib.pvw_shamir_shares_wide_host(None, ptr(one), 1, 0, ptr(pm), None, None, ptr(out)) == 1
    assert lib.pvw_shamir_shares_wide_host(pr._h, ptr(one), 1, 0, ptr(pm), None, None, ptr(out)) == 0
    assert lib.pvw_shamir_reconstruct_wide(None, ptr(one), ptr(one), 1, 1, ptr(out)) == 1
    assert lib.pvw_shamir_wide_from_limbs_host(None, ptr(one), 1, 52, 1, ptr(out)) == 1
    assert lib.pvw_shamir_wide_to_limbs_host(None, 1, 52, 5, ptr(out)) == 1
    # the device entry points check their arguments before any device work
    for name in ("pvw_shamir_shares_wide", "pvw_shamir_shares_wide_device"):
        tail = (None,) if name.endswith("_device") else ()
        assert getattr(lib, name)(pr._h, ptr(one), 1, 0, None, None, None, ptr(out), *tail) == 1
        cp = np.array([(COMPOSITE_255 >> (64 * w)) & (2**64 - 1) for w in range(4)], dtype=np.uint64)
        assert getattr(lib, name)(pr._h, ptr(one), 1, 0, ptr(cp), None, None, ptr(out), *tail) == 1
    assert lib.pvw_selftest_shamir_wide_step(None, ptr(pm), ptr(one), ptr(one), ptr(one), 1, ptr(out)) == 1


def test_p_not_above_n_is_refused():
    pr = params(70)
    with pytest.raises(P.PvwError):
        P.shamir_shares_wide(pr, [1], 0, 67, host=True)
    assert ints(P.shamir_shares_wide(pr, [100], 0, 71, host=True))[0] == [29] * 70


def test_names_and_cpp_mirror():
    for name in ("shamir_shares_wide", "deal_party_shares_wide", "shamir_wide_limbs", "shamir_wide_to_limbs", "shamir_wide_from_limbs",
                 "shamir_reconstruct_wide"):
        assert name in P.__all__ and callable(getattr(P, name))
    for name in ("pvw_shamir_wide_limbs", "pvw_shamir_shares_wide_host", "pvw_shamir_shares_wide_device", "pvw_shamir_shares_wide",
                 "pvw_deal_shares_wide", "pvw_deal_shares_wide_device", "pvw_deal_shares_wide_rs", "pvw_deal_shares_wide_rs_device",
                 "pvw_shamir_wide_to_limbs_host", "pvw_shamir_wide_from_limbs_host", "pvw_shamir_reconstruct_wide",
                 "pvw_selftest_shamir_wide_step"):
        assert name in _ffi._SIGNATURES and hasattr(_ffi.lib(), name)
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr


SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_wide_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])

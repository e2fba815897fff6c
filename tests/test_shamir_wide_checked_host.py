"""Checked Shamir reconstruction over a prime field of up to 256 bits, the CPU half: the general product wide_mul
as a stand-alone program against schoolbook long division; pvw_shamir_reconstruct_wide_checked_host against Python's own
integers (Lagrange with pow(x, -1, p)); the refusals of all three entry points and of the device fold, which are made before
any device work; the names; the C++ mirror.  No device is used."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from test_shamir_wide_host import BLS_R, COMPOSITE_255, PRIMES, SECP_N, W256, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")
P64 = 2**64 + 13
CHECKED_PRIMES = [65537, P64, 2**255 - 19, BLS_R, SECP_N]
PID = lambda p: f"{p.bit_length()}bit"


def lagrange_at(xs, ys, x, p):
    """the value at x of the polynomial through (xs[j], ys[j]) mod p"""
    v = 0
    for j, xj in enumerate(xs):
        num = den = 1
        for i, xi in enumerate(xs):
            if i != j:
                num = num * (x - xi) % p
                den = den * (xj - xi) % p
        v = (v + ys[j] * num * pow(den, -1, p)) % p
    return v


def model(indices, rows, t, p):
    """(secrets, bad, col_bad) of the contract for rows [S][count] of ints (any value, read mod p)"""
    xs = [i + 1 for i in indices]
    count = len(xs)
    out, bad, col_bad = [], [0] * len(rows), [0] * count
    for s, row in enumerate(rows):
        ys = [v % p for v in row]
        out.append(lagrange_at(xs[:t + 1], ys[:t + 1], 0, p))
        for c in range(t + 1, count):
            if lagrange_at(xs[:t + 1], ys[:t + 1], xs[c], p) != ys[c]:
                bad[s] += 1
                col_bad[c] += 1
    return out, bad, col_bad


def sharing(rng, indices, S, t, p):
    """S polynomials of degree <= t with random coefficients, evaluated at the points of `indices`: (secrets, rows [S][count])"""
    secrets, rows = [], []
    for _ in range(S):
        co = [rng.randrange(p) for _ in range(t + 1)]
        secrets.append(co[0])
        rows.append([sum(c * pow(i + 1, e, p) for e, c in enumerate(co)) % p for i in indices])
    return secrets, rows


def checked(indices, rows, t, p, layout="secret_major", pr=None, host=True):
    if layout == "party_major":
        rows = [list(col) for col in zip(*rows)]
    out, bad, col_bad = P.shamir_reconstruct_wide_checked(pr, indices, rows, t, p, host=host, layout=layout)
    return out, bad.tolist(), col_bad.tolist()


def indices_for(rng, count, p):
    top = min(p - 2, 2**64 - 1)                      # the largest legal index: its point is below p
    fixed = [top, 0] if p > 3 else [0]
    idx = fixed[:count]
    while len(idx) < count:
        i = rng.randrange(min(p - 1, 1 << 20))
        if i not in idx:
            idx.append(i)
    return idx


def test_product_against_long_division_under_sanitizers():
    """tests/cpp/shamir_wide_mul.cpp: 10^5 seeded cases per prime of the 13, operands 0, 1, p - 1 and random in every combination
    (the pair (p - 1, p - 1) among them); the unreduced accumulator, the reduction of any four words, addition, subtraction and
    Fermat's inversion ride along"""
    exe = os.path.join(ROOT, "build", "shamir_wide_mul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide_mul.cpp"), "-o", exe])
    assert len(PRIMES) == 13
    out = subprocess.run([exe, "100000"] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_MUL_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_host_form_equals_big_integer_lagrange(p):
    rng = random.Random(p & 0xFFFF)
    for count, t, S in ((7, 3, 4), (9, 0, 3), (6, 5, 2), (12, 4, 5)):
        idx = indices_for(rng, count, p)
        secrets, rows = sharing(rng, idx, S, t, p)
        for layout in ("secret_major", "party_major"):
            out, bad, col_bad = checked(idx, rows, t, p, layout)
            assert out == secrets and bad == [0] * S and col_bad == [0] * count, ("consistent", count, t, layout)
        assert model(idx, rows, t, p) == (secrets, [0] * S, [0] * count)
        if count > t + 1:
            # one wrong extra share: flagged at exactly its (s, c), out stays right
            s, c = rng.randrange(S), rng.randrange(t + 1, count)
            wrong = [list(r) for r in rows]
            wrong[s][c] = (wrong[s][c] + 1 + rng.randrange(p - 1)) % p
            for layout in ("secret_major", "party_major"):
                out, bad, col_bad = checked(idx, wrong, t, p, layout)
                assert out == secrets, ("extra", count, t)
                assert bad == [int(i == s) for i in range(S)] and col_bad == [int(i == c) for i in range(count)], ("extra", count, t, layout)
            # one wrong basis share: out[s] is wrong and every extra of s is flagged
            s, c = rng.randrange(S), rng.randrange(t + 1)
            wrong = [list(r) for r in rows]
            wrong[s][c] = (wrong[s][c] + 1 + rng.randrange(p - 1)) % p
            out, bad, col_bad = checked(idx, wrong, t, p)
            assert out[s] != secrets[s] and [o for i, o in enumerate(out) if i != s] == [o for i, o in enumerate(secrets) if i != s]
            assert bad == [(count - t - 1) * int(i == s) for i in range(S)]
            assert col_bad == [int(i > t) for i in range(count)]
            assert (out, bad, col_bad) == model(idx, wrong, t, p)
        # unreduced words read mod p: v + k p below 2^256, p itself and 2^256 - 1
        un = [[v + p * rng.randrange((W256 - v) // p + 1) for v in r] for r in rows]
        un[0][0], un[0][count - 1] = p, W256
        want = model(idx, un, t, p)
        for layout in ("secret_major", "party_major"):
            assert checked(idx, un, t, p, layout) == want, ("unreduced", count, t, layout)
        # random rows: nothing consistent about them
        rnd = [[rng.getrandbits(256) for _ in range(count)] for _ in range(S)]
        assert checked(idx, rnd, t, p) == model(idx, rnd, t, p), ("random", count, t)


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_no_extras_and_degree_zero(p):
    rng = random.Random(5 + (p & 0xFF))
    idx = indices_for(rng, 5, p)
    secrets, rows = sharing(rng, idx, 3, 4, p)                  # count = degree + 1: no extras
    assert checked(idx, rows, 4, p) == (secrets, [0] * 3, [0] * 5)
    secrets, rows = sharing(rng, idx, 3, 0, p)                  # degree 0: every share is the secret
    assert checked(idx, rows, 0, p) == (secrets, [0] * 3, [0] * 5)
    rows[1][3] = (rows[1][3] + 1) % p
    assert checked(idx, rows, 0, p) == (secrets, [0, 1, 0], [0, 0, 0, 1, 0])
    secrets, rows = sharing(rng, idx[:1], 2, 0, p)              # one share
    assert checked(idx[:1], rows, 0, p) == (secrets, [0, 0], [0])


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_agrees_with_the_plain_wide_reconstruction(p):
    rng = random.Random(9 + (p & 0xFF))
    idx = indices_for(rng, 6, p)[1:] if p > 2**64 else indices_for(rng, 5, p)     # the plain call takes no index of 2^64 - 1
    secrets, rows = sharing(rng, idx, 4, 4, p)
    assert P.shamir_reconstruct_wide(idx, rows, p) == secrets == checked(idx, rows, 4, p)[0]


def test_agrees_with_the_one_word_family_on_a_one_word_prime():
    rng = random.Random(11)
    for p in (65537, 2**61 - 1):
        idx = indices_for(rng, 9, p)
        _, rows = sharing(rng, idx, 4, 3, p)
        rows[2][7] = (rows[2][7] + 5) % p
        rows[1][0] = (rows[1][0] + 5) % p
        for layout in ("secret_major", "party_major"):
            sh = rows if layout == "secret_major" else [list(c) for c in zip(*rows)]
            out, bad, col_bad = P.shamir_reconstruct_checked(None, idx, sh, 3, p, host=True, layout=layout)
            assert checked(idx, rows, 3, p, layout) == (out, bad.tolist(), col_bad.tolist())


def test_an_index_of_2_64_minus_1_needs_p_above_2_64():
    rng = random.Random(13)
    top = 2**64 - 1
    idx = [top, 3, 0]
    secrets, rows = sharing(rng, idx, 2, 1, P64)
    assert checked(idx, rows, 1, P64) == (secrets, [0, 0], [0, 0, 0])
    with pytest.raises(P.PvwError):
        checked(idx, rows, 1, 2**61 - 1)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_refusals_at_all_three_entry_points_and_the_fold():
    """every refusal is made before any device work, so the device entry points are called here without a GPU; nothing is
    written"""
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    count, t, S = 5, 2, 3
    idx = np.arange(count, dtype=np.uint64)
    sh = np.ones((S, count, 4), dtype=np.uint64)
    out = np.full((S, 4), 7, dtype=np.uint64)
    bad, col = np.full(S, 7, dtype=np.uint32), np.full(count, 7, dtype=np.uint32)

    def call(name, pm_=pm, t_=t, idx_=idx, count_=count, sh_=sh, S_=S, ss=count, ps=1, out_=out, ctx=True):
        args = [_ptr(pm_), t_, _ptr(idx_), count_, _ptr(sh_), S_, ss, ps, _ptr(out_), _ptr(bad), _ptr(col)]
        if name != "pvw_shamir_reconstruct_wide_checked_host":
            args = [pr._h if ctx else None] + args
        if name.endswith("_device"):
            args.append(None)
        return getattr(lib, name)(*args)

    w = lambda v: api._wide_modulus(v)
    dup = np.array([0, 1, 2, 1, 4], dtype=np.uint64)
    for name in ("pvw_shamir_reconstruct_wide_checked_host", "pvw_shamir_reconstruct_wide_checked_device", "pvw_shamir_reconstruct_wide_checked"):
        assert call(name, pm_=None) == 1 and call(name, idx_=None) == 1 and call(name, sh_=None) == 1 and call(name, out_=None) == 1, name
        assert call(name, S_=0) == 1, name
        assert call(name, count_=t) == 1 and call(name, t_=count) == 1, name                   # count < degree + 1
        assert call(name, idx_=dup) == 1, name
        assert call(name, pm_=w(5), idx_=np.array([0, 1, 2, 3, 4], dtype=np.uint64)) == 1, name # index 4: the point 5 = p
        assert call(name, pm_=w(2**61 - 1), idx_=np.array([0, 1, 2, 3, 2**61 - 2], dtype=np.uint64)) == 1, name
        assert call(name, pm_=w(2**64 - 59), idx_=np.array([0, 1, 2, 3, 2**64 - 1], dtype=np.uint64)) == 1, name   # the point 2^64 > p
        for bad_p in (COMPOSITE_255, SECP_N - 1, 2**256 - 190, 561, 1, 0, 3 * (2**89 - 1)):
            assert call(name, pm_=w(bad_p)) == 1, (name, bad_p)
        assert call(name, ss=0) == 1 and call(name, ps=0) == 1, name
        if not name.endswith("_host"):
            assert call(name, ctx=False) == 1, name
        assert (out == 7).all() and (bad == 7).all() and (col == 7).all(), name                 # nothing written
    assert call("pvw_shamir_reconstruct_wide_checked_host") == 0 and not (out == 7).all()
    # the fold: the refusals of the host form, a NULL context and a stride of 0
    limbs = np.ones((5, 4), dtype=np.uint64)
    fo = np.zeros((4, 4), dtype=np.uint64)
    fold = lambda ctx=pr._h, pm_=pm, lm=limbs, n=4, ls=4, es=1, lb=52, nl=5, o=fo: lib.pvw_shamir_wide_from_limbs_device(
        ctx, _ptr(pm_), _ptr(lm), n, ls, es, lb, nl, _ptr(o), None)
    assert fold(ctx=None) == 1 and fold(pm_=None) == 1 and fold(lm=None) == 1 and fold(o=None) == 1
    assert fold(lb=15) == 1 and fold(lb=63) == 1 and fold(nl=0) == 1 and fold(nl=17) == 1
    assert fold(pm_=w(COMPOSITE_255)) == 1 and fold(pm_=w(SECP_N - 1)) == 1
    assert fold(ls=0) == 1 and fold(es=0) == 1
    assert not fo.any()
    one = api._wide([1])
    assert lib.pvw_selftest_shamir_wide_mul(None, _ptr(pm), _ptr(one), _ptr(one), 1, _ptr(fo)) == 1
    assert lib.pvw_selftest_shamir_wide_mul(pr._h, _ptr(pm), _ptr(pm), _ptr(one), 1, _ptr(fo)) == 1      # an operand of p


def test_device_forms_refuse_counts_of_2_31_before_any_device_work():
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    idx = np.arange(4, dtype=np.uint64)
    sh = np.ones((2, 4, 4), dtype=np.uint64)
    out = np.zeros((2, 4), dtype=np.uint64)
    for name, tail in (("pvw_shamir_reconstruct_wide_checked_device", (None,)), ("pvw_shamir_reconstruct_wide_checked", ())):
        rc = getattr(lib, name)(pr._h, _ptr(pm), 1, _ptr(idx), 4, _ptr(sh), 1 << 31, 4, 1, _ptr(out), None, None, *tail)
        assert rc == 1 and "2^31" in _ffi.last_error(lib), name
    # count >= 2^31 cannot be reached with a real index array; the bound is one comparison beside the num_secrets one
    assert not out.any()


def test_python_wrapper_refuses_a_ragged_or_misshapen_matrix():
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide_checked(None, [0, 1, 2], [[1, 2, 3], [1, 2]], 1, SECP_N, host=True)
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide_checked(None, [0, 1, 2], [[1, 2], [1, 2]], 1, SECP_N, host=True)
    with pytest.raises(ValueError):
        P.shamir_reconstruct_wide_checked(None, [0, 1], [[1, 2]], 1, SECP_N, host=True, layout="other")
    words = api._wide([5, 5, 5]).reshape(1, 3, 4)
    assert P.shamir_reconstruct_wide_checked(None, [4, 9, 2], words, 0, SECP_N, host=True)[0] == [5]


SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_checked_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_wide_checked_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_names_and_cpp_mirror():
    for name in ("shamir_reconstruct_wide_checked", "shamir_wide_from_limbs_device"):
        assert name in P.__all__ and callable(getattr(P, name))
    for name in ("pvw_shamir_wide_from_limbs_device", "pvw_shamir_reconstruct_wide_checked_host", "pvw_shamir_reconstruct_wide_checked_device",
                 "pvw_shamir_reconstruct_wide_checked", "pvw_selftest_shamir_wide_mul"):
        assert name in _ffi._SIGNATURES and hasattr(_ffi.lib(), name)
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CHECKED_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

"""Corrected Shamir reconstruction over a prime field of up to 256 bits, the CPU half:
pvw_shamir_reconstruct_wide_corrected_host against the contract restated in Python's integers by exhaustive search over all
bases; agreement with the one-word corrected call and with the checked wide call; the refusals of all three entry points, the
locator bound of the device forms included, which are made before any device work; the names; the C++ mirror; and the
Berlekamp-Massey recurrence and the finish formula of the kernels restated sequentially over pvw_wide.h, under the sanitizers,
against Berlekamp-Welch.  No device is used."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from test_shamir_wide_host import COMPOSITE_255, PRIMES, SECP_N, W256, params
from test_shamir_wide_checked_host import CHECKED_PRIMES, PID, indices_for, sharing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")
UNDECODABLE = P.SHAMIR_UNDECODABLE
NAMES = ("pvw_shamir_reconstruct_wide_corrected_host", "pvw_shamir_reconstruct_wide_corrected_device",
         "pvw_shamir_reconstruct_wide_corrected")


def oracle_row(xs, row, t, p):
    """The contract for one row, by exhaustive search: (secret, sorted wrong columns) of the polynomial of degree <= t that is
    off the row in at most E columns, or None.  Every basis of t + 1 columns is tried: a polynomial within E <= r / 2 columns of
    the row agrees with it in at least t + 1 columns, so it is the interpolant of one of them; two such polynomials would agree
    in count - 2 E >= t + 1 columns and be one (asserted for the small cases)."""
    count = len(xs)
    E = (count - t - 1) // 2
    ys = [v % p for v in row]
    found = None
    for basis in itertools.combinations(range(count), t + 1):
        bx = [xs[j] for j in basis]
        w = []
        for j, xj in enumerate(bx):
            den = 1
            for i, xi in enumerate(bx):
                if i != j:
                    den = den * (xj - xi) % p
            w.append(ys[basis[j]] * pow(den, -1, p) % p)

        def at(x):
            v = 0
            for j in range(t + 1):
                num = w[j]
                for i, xi in enumerate(bx):
                    if i != j:
                        num = num * (x - xi) % p
                v += num
            return v % p

        wrong = []
        for c in range(count):
            if c not in basis and at(xs[c]) != ys[c]:
                wrong.append(c)
                if len(wrong) > E:
                    break
        if len(wrong) <= E:
            got = (at(0), wrong)
            if found is None:
                found = got
                if count > 8:
                    break
            else:
                assert got == found, "two polynomials within E"
    return found


def contract(indices, rows, t, p):
    """(secrets, nerr, col_err, mask bits as a set of (s, c)) of the contract for rows [S][count] of ints"""
    xs = [i + 1 for i in indices]
    out, nerr, col_err, bits = [], [], [0] * len(xs), set()
    for s, row in enumerate(rows):
        got = oracle_row(xs, row, t, p)
        if got is None:
            out.append(0)
            nerr.append(UNDECODABLE)
            continue
        out.append(got[0])
        nerr.append(len(got[1]))
        for c in got[1]:
            col_err[c] += 1
            bits.add((s, c))
    return out, nerr, col_err, bits


def corrected(indices, rows, t, p, layout="secret_major"):
    S, count = len(rows), len(indices)
    sh = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, indices, sh, t, p, host=True, layout=layout)
    assert mask.shape == (S, (count + 63) // 64)
    bits = {(s, c) for s in range(S) for c in range(64 * mask.shape[1]) if (int(mask[s][c // 64]) >> (c % 64)) & 1}
    return out, nerr.tolist(), col_err.tolist(), bits


def unreduced(rng, v, p):
    """a word that reads v mod p: v plus a multiple of p, below 2^256"""
    return v + p * rng.randrange((W256 - v) // p + 1)


def spoil(rng, row, cols, p):
    row = list(row)
    for c in cols:
        row[c] = (row[c] + 1 + rng.randrange(p - 1)) % p
    return row


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_host_form_equals_the_contract_by_exhaustive_search(p):
    """t in {0, 1, 2, 5} x r = 0..6, S in {1, 3}, both layouts.  Six rows per shape: consistent; one error inside the first t + 1
    columns; one error anywhere; E errors; E errors with column 0 among them; E + 1 errors -- every row with its own error set,
    every second word unreduced, 2^256 - 1 among them.  The oracle decides what each row is; what was planted is asserted too
    where the contract fixes it (up to E errors: the planted polynomial and exactly the planted columns)."""
    rng = random.Random(p & 0xFFFF)
    for t in (0, 1, 2, 5):
        for r in range(7):
            count, E = t + 1 + r, r // 2
            idx = indices_for(rng, count, p)
            secrets, clean = sharing(rng, idx, 6, t, p)
            plans = [[], [rng.randrange(t + 1)], [rng.randrange(count)], rng.sample(range(count), E),
                     sorted({0} | set(rng.sample(range(1, count), max(E - 1, 0)))) if E else [], rng.sample(range(count), E + 1)]
            rows = [spoil(rng, clean[s], plans[s], p) for s in range(6)]
            rows = [[unreduced(rng, v, p) if (s + c) % 2 else v for c, v in enumerate(row)] for s, row in enumerate(rows)]
            rows[5][count - 1] = W256                           # 2^256 - 1: whatever it reads as, the oracle reads the same
            want = [contract(idx, [row], t, p) for row in rows]
            for s in range(5):
                if len(plans[s]) <= E:
                    assert want[s][0] == [secrets[s]] and want[s][3] == {(0, c) for c in plans[s]}, ("planted", t, r, s)
            if r == 1:
                assert all(w[1] == [UNDECODABLE] for s, w in enumerate(want) if plans[s] and s < 5), ("detects only", t, r)
            for s, row in enumerate(rows):                      # S = 1, the layouts in turn
                assert corrected(idx, [row], t, p, ("secret_major", "party_major")[s % 2]) == want[s], ("S=1", t, r, s)
            for s0 in (0, 3):                                   # S = 3, both layouts
                exp_out = [want[s][0][0] for s in range(s0, s0 + 3)]
                exp_nerr = [want[s][1][0] for s in range(s0, s0 + 3)]
                exp_col = [sum(want[s][2][c] for s in range(s0, s0 + 3)) for c in range(count)]
                exp_bits = {(s - s0, c) for s in range(s0, s0 + 3) for (_, c) in want[s][3]}
                for layout in ("secret_major", "party_major"):
                    got = corrected(idx, rows[s0:s0 + 3], t, p, layout)
                    assert got == (exp_out, exp_nerr, exp_col, exp_bits), ("S=3", t, r, s0, layout)


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_a_whole_bad_column_in_every_position_and_the_order_of_the_columns(p):
    rng = random.Random(3 + (p & 0xFF))
    t, count, S = 2, 7, 3                                       # r = 4, E = 2
    idx = indices_for(rng, count, p)
    secrets, clean = sharing(rng, idx, S, t, p)
    for c in range(count):
        rows = [spoil(rng, row, [c], p) for row in clean]
        got = corrected(idx, rows, t, p)
        assert got == (secrets, [1] * S, [S * int(i == c) for i in range(count)], {(s, c) for s in range(S)}), c
        assert got == contract(idx, rows, t, p), c
    # another error set in every row, then the columns in another order: the same secrets, the bits and counts move along
    sets = [[0, 5], [1], [2, 6]]
    rows = [spoil(rng, row, sets[s], p) for s, row in enumerate(clean)]
    base = corrected(idx, rows, t, p)
    assert base[0] == secrets and base[3] == {(s, c) for s in range(S) for c in sets[s]}
    perm = list(range(count))
    rng.shuffle(perm)
    got = corrected([idx[c] for c in perm], [[row[c] for c in perm] for row in rows], t, p, "party_major")
    assert got[0] == base[0] and got[1] == base[1]
    assert got[2] == [base[2][c] for c in perm] and got[3] == {(s, perm.index(c)) for (s, c) in base[3]}


def test_agrees_with_the_one_word_corrected_call_on_a_one_word_prime():
    rng = random.Random(11)
    for p in (65537, 2**61 - 1):
        for t, count in ((3, 9), (0, 4), (2, 3), (1, 8)):
            idx = indices_for(rng, count, p)
            E = (count - t - 1) // 2
            _, rows = sharing(rng, idx, 4, t, p)
            rows[0] = spoil(rng, rows[0], rng.sample(range(count), E), p)
            rows[1] = spoil(rng, rows[1], rng.sample(range(count), E + 1), p)
            rows[2] = [rng.randrange(p) for _ in range(count)]
            for layout in ("secret_major", "party_major"):
                sh = rows if layout == "secret_major" else [list(c) for c in zip(*rows)]
                a = P.shamir_reconstruct_corrected(None, idx, sh, t, p, host=True, layout=layout)
                b = P.shamir_reconstruct_wide_corrected(None, idx, sh, t, p, host=True, layout=layout)
                assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), (p, t, count, layout)


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_agrees_with_the_checked_wide_call_on_consistent_shares(p):
    rng = random.Random(9 + (p & 0xFF))
    for t, count in ((4, 5), (2, 9), (0, 1)):
        idx = indices_for(rng, count, p)
        secrets, rows = sharing(rng, idx, 4, t, p)
        out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, idx, rows, t, p, host=True)
        assert out == secrets == P.shamir_reconstruct_wide_checked(None, idx, rows, t, p, host=True)[0]
        assert not nerr.any() and not col_err.any() and not mask.any()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_refusals_at_all_three_entry_points():
    """every refusal is made before any device work, so the device entry points are called here without a GPU; nothing is
    written.  The order and the cases are those of the checked wide call; the device forms add the locator bound."""
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    count, t, S = 5, 2, 3
    idx = np.arange(count, dtype=np.uint64)
    sh = np.ones((S, count, 4), dtype=np.uint64)
    out = np.full((S, 4), 7, dtype=np.uint64)
    nerr, col, mask = np.full(S, 7, dtype=np.uint32), np.full(count, 7, dtype=np.uint32), np.full((S, 1), 7, dtype=np.uint64)

    def call(name, pm_=pm, t_=t, idx_=idx, count_=count, sh_=sh, S_=S, ss=count, ps=1, out_=out, ctx=True):
        args = [_ptr(pm_), t_, _ptr(idx_), count_, _ptr(sh_), S_, ss, ps, _ptr(out_), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h if ctx else None] + args
        if name.endswith("_device"):
            args.append(None)
        return getattr(lib, name)(*args)

    w = lambda v: api._wide_modulus(v)
    dup = np.array([0, 1, 2, 1, 4], dtype=np.uint64)
    for name in NAMES:
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
        assert (out == 7).all() and (nerr == 7).all() and (col == 7).all() and (mask == 7).all(), name   # nothing written
    # the order: a duplicate is reported before a composite modulus, as by the checked call
    assert call(NAMES[0], idx_=dup, pm_=w(561)) == 1 and "duplicate" in _ffi.last_error(lib)
    assert call(NAMES[0]) == 0 and not (out == 7).all()


def test_device_forms_refuse_counts_of_2_31_and_a_locator_above_the_bound_before_any_device_work():
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    big = 2 * 2048 + 1                                          # t = 0: r = 4096, E + 1 = 2049
    idx = np.arange(big, dtype=np.uint64)
    sh = np.ones((1, big, 4), dtype=np.uint64)
    out = np.full((2, 4), 7, dtype=np.uint64)
    for name, tail in ((NAMES[1], (None,)), (NAMES[2], ())):
        rc = getattr(lib, name)(pr._h, _ptr(pm), 1, _ptr(idx), 4, _ptr(sh), 1 << 31, 4, 1, _ptr(out), None, None, None, *tail)
        assert rc == 1 and "2^31" in _ffi.last_error(lib), name
        rc = getattr(lib, name)(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, big, 1, _ptr(out), None, None, None, *tail)
        assert rc == 1 and "locator" in _ffi.last_error(lib) and "2048" in _ffi.last_error(lib), name
        # the argument checks come first: the same call with a stride of 0 is refused for the stride
        rc = getattr(lib, name)(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, 0, 1, _ptr(out), None, None, None, *tail)
        assert rc == 1 and "stride" in _ffi.last_error(lib), name
    assert (out == 7).all()


def test_python_wrapper_refuses_a_ragged_or_misshapen_matrix():
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide_corrected(None, [0, 1, 2], [[1, 2, 3], [1, 2]], 1, SECP_N, host=True)
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide_corrected(None, [0, 1, 2], [[1, 2], [1, 2]], 1, SECP_N, host=True)
    with pytest.raises(ValueError):
        P.shamir_reconstruct_wide_corrected(None, [0, 1], [[1, 2]], 1, SECP_N, host=True, layout="other")
    words = api._wide([5, 5, 6]).reshape(1, 3, 4)               # degree 0, r = 2: one error corrected
    out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, [4, 9, 2], words, 0, SECP_N, host=True)
    assert out == [5] and nerr.tolist() == [1] and col_err.tolist() == [0, 0, 1] and mask.tolist() == [[4]]


SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_corrected_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_wide_corrected_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_names_and_cpp_mirror():
    assert "shamir_reconstruct_wide_corrected" in P.__all__ and callable(P.shamir_reconstruct_wide_corrected)
    for name in NAMES:
        assert name in _ffi._SIGNATURES and hasattr(_ffi.lib(), name)
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CORRECTED_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr


def test_kernel_recurrence_against_berlekamp_welch_under_sanitizers():
    """tests/cpp/shamir_wide_corrected.cpp: the inversion-free Berlekamp-Massey recurrence and the finish formula in the kernels'
    update order and forms, sequentially, over pvw_wide.h's own product, accumulator and reduction, against Berlekamp-Welch by
    Gaussian elimination on seeded rows with 0 .. E + 1 errors, for each of the 13 primes.  The only sanitizer run: nothing
    loaded into Python is sanitized."""
    exe = os.path.join(ROOT, "build", "shamir_wide_corrected")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide_corrected.cpp"), "-o", exe])
    assert len(PRIMES) == 13
    out = subprocess.run([exe, "40"] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CORRECTED_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

"""Corrected Shamir reconstruction on the host side: pvw_shamir_reconstruct_corrected_host (Berlekamp-Welch by
Gaussian elimination) against the contract restated in Python integers by exhaustive search for the nearest polynomial, the
refusals at all three entry points (the device ones refuse without a GPU), agreement with the checked routine on consistent
shares, and the C++ mirror.  No device compute here; the kernels are checked against the host routine in
tests/test_gpu_shamir_correct.py.

The grid: t in {0, 1, 2, 5}, r = count - t - 1 in 0..6 (count <= 8 where the search is exhaustive over all bases, which it is
for every shape here: at most C(12, 6) bases), S in {1, 3}, both layouts, scattered indices with one near 2^40, unreduced words,
p in {257, 65537, 2^61 - 1, 2^62 - 57}; 0, 1, E and E + 1 errors per row, errors inside the first t + 1 columns, rows with
different error sets, a whole bad column."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _shamir_correct_util import (P61, P62, U64, UNDECODABLE, bend, indices_for, mask_ints, restated, sharing, unreduce)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS = 1
PRIMES = (257, 65537, P61, P62)
NEW = ["pvw_shamir_reconstruct_corrected_host", "pvw_shamir_reconstruct_corrected_device", "pvw_shamir_reconstruct_corrected"]


def corrected_host(indices, rows, t, p, layout="secret_major"):
    """through the Python mirror, rows given secret-major and handed over in `layout`"""
    arr = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    out, nerr, col_err, mask = P.shamir_reconstruct_corrected(None, indices, arr, t, p, host=True, layout=layout)
    return out, nerr.tolist(), col_err.tolist(), mask_ints(mask)


def test_both_libraries_export_the_entry_points_and_the_constant():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name
    assert "#define PVW_SHAMIR_UNDECODABLE 0xFFFFFFFFu" in header and P.SHAMIR_UNDECODABLE == UNDECODABLE


def error_sets(t, count, E, S, rng):
    """per case one list of error columns per row: none; one; E; E + 1; only inside columns 0..t; different sets per row"""
    cols = list(range(count))
    cases = [[[] for _ in range(S)]]
    if E >= 1:
        cases.append([[rng.randrange(count)] for _ in range(S)])
        cases.append([rng.sample(cols, E) for _ in range(S)])
        cases.append([rng.sample(cols[:t + 1], min(E, t + 1)) for _ in range(S)])
        cases.append([rng.sample(cols, rng.randrange(E + 1)) for _ in range(S)])
    if E + 1 <= count:
        cases.append([rng.sample(cols, E + 1) if s % 2 == 0 else rng.sample(cols, E) for s in range(S)])
    return cases


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("t", [0, 1, 2, 5])
def test_host_equals_the_restatement(t, p):
    rng = random.Random(1000 * t + p % 101)
    for r in range(0, 7):
        count = t + 1 + r
        E = r // 2
        for S in (1, 3):
            idx = indices_for(count, p, rng)
            secrets, rows = sharing(idx, t, p, S, rng)
            for case in error_sets(t, count, E, S, rng):
                bent = [list(row) for row in rows]
                for s, cols in enumerate(case):
                    bend(bent, s, cols, p, rng)
                want = restated(idx, bent, t, p)
                words = unreduce(bent, p, rng)
                for layout in ("secret_major", "party_major"):
                    assert corrected_host(idx, words, t, p, layout) == want, (t, p, r, S, case, layout)
                # within E planted errors the dealt secret comes back and exactly the planted columns are named
                for s, cols in enumerate(case):
                    if len(cols) <= E:
                        assert want[0][s] == secrets[s] and want[1][s] == len(cols) and want[3][s] == sum(1 << c for c in cols)
                    elif p > 65537 and r >= 1:            # r = 0: every row is a polynomial; else a false decode has probability about count^E / p
                        assert want[1][s] == UNDECODABLE and want[0][s] == 0 and want[3][s] == 0


@pytest.mark.parametrize("p", PRIMES)
def test_arbitrary_words_also_where_a_far_row_decodes_to_another_polynomial(p):
    """rows of arbitrary 64-bit words: at p = 257 some lie within E of a polynomial nobody dealt, and the host finds it"""
    rng = random.Random(p % 313)
    decoded = 0
    # t = 0, count = 3: two equal words of three decode to that constant, about 3 / p of the rows
    for t, count, S in ((0, 3, 300 if p == 257 else 12), (0, 5, 12), (1, 6, 12), (1, 7, 12), (2, 8, 12)):
        idx = indices_for(count, p, rng)
        rows = [[rng.getrandbits(64) for _ in idx] for _ in range(S)]
        want = restated(idx, rows, t, p)
        assert corrected_host(idx, rows, t, p) == want
        decoded += sum(n != UNDECODABLE for n in want[1])
    if p == 257:
        assert decoded > 0
    if p > 65537:
        assert decoded == 0


@pytest.mark.parametrize("p", PRIMES)
def test_a_whole_bad_column_is_named_whichever_column_it_is(p):
    rng = random.Random(p % 211)
    t, count, S = 2, 7, 3                                # r = 4, E = 2
    idx = indices_for(count, p, rng)
    secrets, rows = sharing(idx, t, p, S, rng)
    for c in range(count):                               # columns 0..t included: no column is a basis
        bent = [list(r) for r in rows]
        for s in range(S):
            bend(bent, s, [c], p, rng)
        for layout in ("secret_major", "party_major"):
            out, nerr, col_err, masks = corrected_host(idx, bent, t, p, layout)
            assert out == secrets and nerr == [1] * S and masks == [1 << c] * S
            assert col_err == [S * int(i == c) for i in range(count)]


def test_column_order_changes_no_output():
    rng = random.Random(77)
    t, count, S, p = 2, 8, 3, P61
    idx = indices_for(count, p, rng)
    _, rows = sharing(idx, t, p, S, rng)
    bend(rows, 0, [0, 5], p, rng), bend(rows, 2, [1], p, rng), bend(rows, 1, [0, 1, 2], p, rng)
    base = corrected_host(idx, rows, t, p)
    assert base[1] == [2, UNDECODABLE, 1]
    for _ in range(5):
        perm = list(range(count))
        rng.shuffle(perm)
        out, nerr, col_err, masks = corrected_host([idx[c] for c in perm], [[row[c] for c in perm] for row in rows], t, p)
        assert out == base[0] and nerr == base[1]
        assert col_err == [base[2][c] for c in perm]
        assert masks == [sum(((mk >> c) & 1) << i for i, c in enumerate(perm)) for mk in base[3]]


def test_on_consistent_shares_out_is_that_of_the_checked_routine():
    rng = random.Random(5)
    for p in PRIMES:
        for t, count in ((0, 1), (1, 2), (1, 6), (5, 6), (5, 12), (9, 30)):
            idx = indices_for(count, p, rng)
            _, rows = sharing(idx, t, p, 4, rng)
            words = unreduce(rows, p, rng)
            out, nerr, col_err, masks = corrected_host(idx, words, t, p)
            chk, bad, col_bad = P.shamir_reconstruct_checked(None, idx, words, t, p, host=True)
            assert out == chk and nerr == [0] * 4 and col_err == [0] * count and masks == [0] * 4
            assert not bad.any() and not col_bad.any()


def test_no_redundancy_interpolates_and_one_redundant_column_only_detects():
    rng = random.Random(6)
    p, t = P62, 3
    idx = indices_for(t + 2, p, rng)
    rows = [[rng.getrandbits(64) for _ in range(t + 1)] for _ in range(3)]
    out, nerr, _, _ = corrected_host(idx[:t + 1], rows, t, p)
    assert out == P.shamir_reconstruct(idx[:t + 1], rows, p) and nerr == [0] * 3
    secrets, rows = sharing(idx, t, p, 2, rng)
    bend(rows, 1, [2], p, rng)
    out, nerr, col_err, masks = corrected_host(idx, rows, t, p)
    assert out == [secrets[0], 0] and nerr == [0, UNDECODABLE] and col_err == [0] * (t + 2) and masks == [0, 0]


def _rc(p=P61, t=2, idx=(0, 7, 3, 999, 12), S=2, ss=None, ps=1, shares=True, out=True, indices=True, name="host", ctx=None):
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ix = np.array(idx, dtype=np.uint64)
    count = len(ix)
    sh = np.arange(max(1, S * max(count, 1)), dtype=np.uint64)
    o = np.full(max(S, 1), 77, dtype=np.uint64)
    nerr = np.full(max(S, 1), 77, dtype=np.uint32)
    col = np.full(max(count, 1), 77, dtype=np.uint32)
    mask = np.full(max(S, 1) * ((count + 63) // 64 + 1), 77, dtype=np.uint64)
    args = [p, t, ptr(ix) if indices else None, count, ptr(sh) if shares else None, S, count if ss is None else ss, ps,
            ptr(o) if out else None, ptr(nerr), ptr(col), ptr(mask)]
    if name == "host":
        rc = lib.pvw_shamir_reconstruct_corrected_host(*args)
    elif name == "buffers":
        rc = lib.pvw_shamir_reconstruct_corrected(ctx, *args)
    else:
        rc = lib.pvw_shamir_reconstruct_corrected_device(ctx, *args, None)
    if rc != 0:
        assert (o == 77).all() and (nerr == 77).all() and (col == 77).all() and (mask == 77).all(), "a refused call writes nothing"
    return rc


REJECTED = [
    dict(indices=False), dict(shares=False), dict(out=False),                  # NULL arguments
    dict(S=0),                                                                 # no secrets
    dict(t=5), dict(t=7), dict(idx=()),                                        # count < degree + 1
    dict(idx=(0, 7, 3, 7, 12)),                                                # duplicate
    dict(p=65537, idx=(0, 1, 2, 3, 65536)), dict(idx=(0, 1, 2, 3, U64)),       # index >= p - 1
    dict(p=561), dict(p=3215031751), dict(p=3825123056546413051), dict(p=65537 * 65537), dict(p=0), dict(p=1),   # composite
    dict(p=1 << 62), dict(p=(1 << 62) + 135), dict(p=U64),                     # p >= 2^62
    dict(ss=0), dict(ps=0),                                                    # a stride of 0
]


def test_rejections():
    assert _rc() == 0
    assert _rc(t=4) == 0 and _rc(p=65537, idx=(0, 1, 2, 3, 65535)) == 0
    for kw in REJECTED:
        assert _rc(**kw) == INVALID_PARAMETERS, kw
    # nerr, col_err and err_mask are optional
    lib = _ffi.lib()
    ix, sh, o = np.array([4, 1, 9], dtype=np.uint64), np.array([5, 5, 5], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pvw_shamir_reconstruct_corrected_host(P61, 0, ptr(ix), 3, ptr(sh), 1, 3, 1, ptr(o), None, None, None) == 0 and o[0] == 5


def test_device_entry_points_refuse_the_same_arguments_before_any_device_work():
    """no GPU is needed to be refused; on the device the locator is bounded as well (E + 1 <= 4096)"""
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    for name in ("buffers", "device"):
        for kw in REJECTED:
            assert _rc(name=name, ctx=prm._h, **kw) == INVALID_PARAMETERS, (name, kw)
        assert _rc(name=name, ctx=None) == INVALID_PARAMETERS
        assert _rc(name=name, ctx=prm._h, t=0, S=1, idx=tuple(range(8193))) == INVALID_PARAMETERS      # r = 8192: E + 1 = 4097


def test_device_forms_refuse_2_31_secrets_and_name_the_locator_bound_before_any_device_work():
    """the kernels' 32-bit counts: refused before the shares are read (the array behind the count holds two rows); the locator
    bound's own text"""
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    ix, sh, o = np.arange(4, dtype=np.uint64), np.ones(8, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    for name, tail in (("pvw_shamir_reconstruct_corrected_device", (None,)), ("pvw_shamir_reconstruct_corrected", ())):
        rc = getattr(lib, name)(prm._h, P61, 1, ptr(ix), 4, ptr(sh), 1 << 31, 4, 1, ptr(o), None, None, None, *tail)
        assert rc == INVALID_PARAMETERS and "2^31" in _ffi.last_error(lib), name
    assert not o.any()
    for name in ("buffers", "device"):
        assert _rc(name=name, ctx=prm._h, t=0, S=1, idx=tuple(range(8193))) == INVALID_PARAMETERS
        text = _ffi.last_error(lib)
        assert "locator" in text and "4096" in text and "8192" in text and "wide" not in text and "erasures" not in text, name


# ---- C++ mirror -------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "reconstruct_corrected.cpp")
EXE = os.path.join(ROOT, "build", "reconstruct_corrected_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_corrects_and_reports_on_the_host():
    """pvw_host::shamir_reconstruct_corrected(host = true) needs no GPU: the program's host half runs everywhere"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CORRECT_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

"""Share repair on the host side: pvw_shamir_evaluate_corrected_host (Berlekamp-Welch, the quotient evaluated by
Horner's rule) against the contract restated in Python integers -- the exhaustive search of _shamir_correct_util finds each
row's polynomial, which is then evaluated at the targets -- the agreement of out, nerr, col_err and err_mask with the corrected
call, the refusals at all three entry points (the device ones refuse without a GPU) and the C++ mirror.  No device compute here;
the kernels are checked against the host routine in tests/test_gpu_shamir_evaluate.py.

The grid is that of tests/test_shamir_correct_host.py: t in {0, 1, 2, 5}, r in 0..6, S in {1, 3}, both layouts, scattered
indices, unreduced words, p in {257, 65537, 2^61 - 1, 2^62 - 57}; 0, 1, E and E + 1 errors per row, rows with different error
sets, a whole bad column, arbitrary words.  Targets: none of the points (T = 1, 2, 7), all columns in order, only the wrong
columns, only right columns, duplicates, a shuffled mix."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _shamir_correct_util import (P61, P62, U64, UNDECODABLE, bend, indices_for, mask_ints, sharing, unreduce)
from _shamir_evaluate_util import off_points, restated_values, target_mixes
from test_shamir_correct_host import REJECTED, error_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS = 1
PRIMES = (257, 65537, P61, P62)
NEW = ["pvw_shamir_evaluate_corrected_host", "pvw_shamir_evaluate_corrected_device", "pvw_shamir_evaluate_corrected"]


def evaluated_host(indices, rows, t, p, targets, layout="secret_major"):
    """through the Python mirror, rows given secret-major and handed over in `layout`: (values, (out, nerr, col_err, masks))"""
    arr = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    values, out, nerr, col_err, mask = P.shamir_evaluate_corrected(None, indices, arr, t, p, targets, host=True, layout=layout)
    return values.tolist(), (out, nerr.tolist(), col_err.tolist(), mask_ints(mask))


def corrected_host(indices, rows, t, p):
    out, nerr, col_err, mask = P.shamir_reconstruct_corrected(None, indices, rows, t, p, host=True)
    return out, nerr.tolist(), col_err.tolist(), mask_ints(mask)


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name
    assert "shamir_evaluate_corrected" in P.__all__
    assert "corrected share values are not returned" not in header


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("t", [0, 1, 2, 5])
def test_host_equals_the_restatement(t, p):
    rng = random.Random(2000 * t + p % 103)
    seen = set()
    for r in range(0, 7):
        count = t + 1 + r
        E = r // 2
        for S in (1, 3):
            idx = indices_for(count, p, rng)
            _, rows = sharing(idx, t, p, S, rng)
            for case in error_sets(t, count, E, S, rng):
                bent = [list(row) for row in rows]
                for s, cols in enumerate(case):
                    bend(bent, s, cols, p, rng)
                words = unreduce(bent, p, rng)
                wrong = set(c for cols in case for c in cols)
                mixes = target_mixes(idx, wrong, p, rng)
                seen.update(mixes)
                for name, targets in mixes.items():
                    want = restated_values(idx, bent, t, p, targets)
                    for layout in ("secret_major", "party_major"):
                        got = evaluated_host(idx, words, t, p, targets, layout)
                        assert got == want, (t, p, r, S, case, name, layout)
                    # the four reports are the corrected call's
                    assert got[1] == corrected_host(idx, words, t, p)
                    for s, cols in enumerate(case):
                        if len(cols) <= E:
                            # within E planted errors the values are the DEALT shares: at a wrong column what the party should hold,
                            # at a right column the share read mod p
                            for j, tg in enumerate(targets):
                                if tg in idx:
                                    assert got[0][s][j] == rows[s][idx.index(tg)], (t, p, r, s, name)
                        elif got[1][1][s] == UNDECODABLE:
                            assert got[0][s] == [0] * len(targets)
                        if got[1][1][s] != UNDECODABLE:
                            for j, tg in enumerate(targets):
                                if tg in idx and not (got[1][3][s] >> idx.index(tg)) & 1:
                                    assert got[0][s][j] == bent[s][idx.index(tg)]
    assert {"columns", "off1", "off2", "off7", "wrong", "right", "duplicates", "mixed7"} <= seen


@pytest.mark.parametrize("p", PRIMES)
def test_arbitrary_words_also_where_a_far_row_decodes_to_another_polynomial(p):
    """rows of arbitrary 64-bit words: at p = 257 some lie within E of a polynomial nobody dealt, and its values are returned"""
    rng = random.Random(p % 317)
    decoded = 0
    for t, count, S in ((0, 3, 300 if p == 257 else 12), (0, 5, 12), (1, 6, 12), (1, 7, 12), (2, 8, 12)):
        idx = indices_for(count, p, rng)
        rows = [[rng.getrandbits(64) for _ in idx] for _ in range(S)]
        targets = list(idx) + off_points(idx, p, 3, rng)
        rng.shuffle(targets)
        want = restated_values(idx, rows, t, p, targets)
        assert evaluated_host(idx, rows, t, p, targets) == want
        decoded += sum(n != UNDECODABLE for n in want[1][1])
        for s, n in enumerate(want[1][1]):
            if n == UNDECODABLE:
                assert want[0][s] == [0] * len(targets)
    if p == 257:
        assert decoded > 0
    if p > 65537:
        assert decoded == 0


@pytest.mark.parametrize("p", PRIMES)
def test_a_whole_bad_column_is_repaired_whichever_column_it_is(p):
    rng = random.Random(p % 223)
    t, count, S = 2, 7, 3                                # r = 4, E = 2
    idx = indices_for(count, p, rng)
    _, rows = sharing(idx, t, p, S, rng)
    for c in range(count):
        bent = [list(r) for r in rows]
        for s in range(S):
            bend(bent, s, [c], p, rng)
        for layout in ("secret_major", "party_major"):
            values, report = evaluated_host(idx, bent, t, p, [idx[c]] + list(idx), layout)
            assert [v[0] for v in values] == [row[c] for row in rows]
            assert [v[1:] for v in values] == rows and report[2] == [S * int(i == c) for i in range(count)]


def test_column_order_changes_no_value_and_target_order_permutes_the_columns():
    rng = random.Random(78)
    t, count, S, p = 2, 8, 3, P61
    idx = indices_for(count, p, rng)
    _, rows = sharing(idx, t, p, S, rng)
    bend(rows, 0, [0, 5], p, rng), bend(rows, 2, [1], p, rng), bend(rows, 1, [0, 1, 2], p, rng)
    targets = [idx[0], idx[5], idx[3]] + off_points(idx, p, 3, rng) + [idx[0]]
    base_values, base = evaluated_host(idx, rows, t, p, targets)
    assert base[1] == [2, UNDECODABLE, 1] and base_values[1] == [0] * len(targets)
    for _ in range(5):
        perm = list(range(count))
        rng.shuffle(perm)
        values, report = evaluated_host([idx[c] for c in perm], [[row[c] for c in perm] for row in rows], t, p, targets)
        assert values == base_values and report[0] == base[0] and report[1] == base[1]
        tperm = list(range(len(targets)))
        rng.shuffle(tperm)
        values, report = evaluated_host(idx, rows, t, p, [targets[j] for j in tperm])
        assert values == [[row[j] for j in tperm] for row in base_values] and report == base


def test_no_redundancy_interpolates_and_one_redundant_column_only_detects():
    rng = random.Random(8)
    p, t = P62, 3
    idx = indices_for(t + 2, p, rng)
    rows = [[rng.getrandbits(64) for _ in range(t + 1)] for _ in range(3)]
    targets = idx[:t + 1] + off_points(idx, p, 2, rng)
    values, report = evaluated_host(idx[:t + 1], rows, t, p, targets)
    assert values == restated_values(idx[:t + 1], rows, t, p, targets)[0] and report[1] == [0] * 3
    assert [v[:t + 1] for v in values] == [[w % p for w in row] for row in rows]
    _, rows = sharing(idx, t, p, 2, rng)
    clean = list(rows[1])
    bend(rows, 1, [2], p, rng)
    values, report = evaluated_host(idx, rows, t, p, idx)
    assert values == [rows[0], [0] * (t + 2)] and report[1] == [0, UNDECODABLE] and clean != rows[1]


def _rc(p=P61, t=2, idx=(0, 7, 3, 999, 12), S=2, ss=None, ps=1, shares=True, out=True, indices=True, name="host", ctx=None,
        targets=(7, 5, 7), values=True, tgt=True, T=None):
    """as test_shamir_correct_host._rc: `out=False` withholds values (the argument that may not be NULL here)"""
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ix = np.array(idx, dtype=np.uint64)
    tg = np.array(targets, dtype=np.uint64)
    count = len(ix)
    nT = len(tg) if T is None else T
    sh = np.arange(max(1, S * max(count, 1)), dtype=np.uint64)
    v = np.full(max(S, 1) * max(len(tg), 1), 77, dtype=np.uint64)
    o = np.full(max(S, 1), 77, dtype=np.uint64)
    nerr = np.full(max(S, 1), 77, dtype=np.uint32)
    col = np.full(max(count, 1), 77, dtype=np.uint32)
    mask = np.full(max(S, 1) * ((count + 63) // 64 + 1), 77, dtype=np.uint64)
    args = [p, t, ptr(ix) if indices else None, count, ptr(sh) if shares else None, S, count if ss is None else ss, ps,
            ptr(tg) if tgt else None, nT, ptr(v) if (values and out) else None, ptr(o), ptr(nerr), ptr(col), ptr(mask)]
    if name == "host":
        rc = lib.pvw_shamir_evaluate_corrected_host(*args)
    elif name == "buffers":
        rc = lib.pvw_shamir_evaluate_corrected(ctx, *args)
    else:
        rc = lib.pvw_shamir_evaluate_corrected_device(ctx, *args, None)
    if rc != 0:
        assert (v == 77).all() and (o == 77).all() and (nerr == 77).all() and (col == 77).all() and (mask == 77).all(), "a refused call writes nothing"
    return rc


OWN_REJECTED = [
    dict(tgt=False), dict(values=False),                                       # NULL targets / values
    dict(T=0),                                                                 # no targets
    dict(p=65537, idx=(0, 1, 2, 3, 4), targets=(9, 65536)), dict(targets=(P61 - 1,)), dict(targets=(3, U64)),   # a target >= p - 1
]


def test_rejections():
    assert _rc() == 0
    assert _rc(p=65537, idx=(0, 1, 2, 3, 4), targets=(9, 65535)) == 0 and _rc(targets=(P61 - 2,)) == 0
    for kw in REJECTED + OWN_REJECTED:
        assert _rc(**kw) == INVALID_PARAMETERS, kw
    # out, nerr, col_err and err_mask are optional
    lib = _ffi.lib()
    ix, sh, tg = np.array([4, 1, 9], dtype=np.uint64), np.array([5, 5, 5], dtype=np.uint64), np.array([100, 1], dtype=np.uint64)
    v = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pvw_shamir_evaluate_corrected_host(P61, 0, ptr(ix), 3, ptr(sh), 1, 3, 1, ptr(tg), 2, ptr(v), None, None, None, None) == 0
    assert v.tolist() == [5, 5]


def test_device_entry_points_refuse_the_same_arguments_before_any_device_work():
    """no GPU is needed to be refused; on the device the locator and the number of targets are bounded as well"""
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    for name in ("buffers", "device"):
        for kw in REJECTED + OWN_REJECTED:
            assert _rc(name=name, ctx=prm._h, **kw) == INVALID_PARAMETERS, (name, kw)
        assert _rc(name=name, ctx=None) == INVALID_PARAMETERS
        assert _rc(name=name, ctx=prm._h, t=0, S=1, idx=tuple(range(8193))) == INVALID_PARAMETERS      # r = 8192: E + 1 = 4097
        # num_targets >= 2^31 is refused before the targets are read: the array behind the count holds three
        for T in (1 << 31, (1 << 31) + 5, 1 << 40):
            assert _rc(name=name, ctx=prm._h, T=T) == INVALID_PARAMETERS, (name, T)
            assert "num_targets" in _ffi.last_error(_ffi.lib()), (name, T)


def test_device_forms_refuse_2_31_secrets_and_name_the_locator_bound_before_any_device_work():
    """the kernels' 32-bit counts: refused before the shares are read (the array behind the count holds two rows); the locator
    bound is the corrected call's, with its text, and comes behind the bound on num_targets"""
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    ix, sh, tg, v = np.arange(4, dtype=np.uint64), np.ones(8, dtype=np.uint64), np.array([9], dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    for name, tail in (("pvw_shamir_evaluate_corrected_device", (None,)), ("pvw_shamir_evaluate_corrected", ())):
        rc = getattr(lib, name)(prm._h, P61, 1, ptr(ix), 4, ptr(sh), 1 << 31, 4, 1, ptr(tg), 1, ptr(v), None, None, None, None, *tail)
        assert rc == INVALID_PARAMETERS and "2^31" in _ffi.last_error(lib) and "num_targets" not in _ffi.last_error(lib), name
    assert not v.any()
    for name in ("buffers", "device"):
        assert _rc(name=name, ctx=prm._h, t=0, S=1, idx=tuple(range(8193))) == INVALID_PARAMETERS
        text = _ffi.last_error(lib)
        assert "locator" in text and "4096" in text and "8192" in text and "wide" not in text and "erasures" not in text, name
        assert _rc(name=name, ctx=prm._h, t=0, S=1, idx=tuple(range(8193)), T=1 << 31) == INVALID_PARAMETERS
        assert "num_targets" in _ffi.last_error(lib), name


def test_the_bound_on_the_targets_is_the_device_forms_alone():
    """the host routine has no 32-bit count: a num_targets it can walk is taken whatever its size class (the header says it reads
    every target, so 2^31 itself is not tried here), and an out-of-range target behind a device-refused count is never reached"""
    assert _rc(targets=tuple(range(20, 20 + 70000))) == 0
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    for name in ("buffers", "device"):
        assert _rc(name=name, ctx=prm._h, targets=(U64, U64, U64), T=1 << 31) == INVALID_PARAMETERS
        assert "num_targets" in _ffi.last_error(_ffi.lib())


# ---- C++ mirror -------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "evaluate_corrected.cpp")
EXE = os.path.join(ROOT, "build", "evaluate_corrected_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_repairs_shares_on_the_host():
    """pvw_host::shamir_evaluate_corrected(host = true) needs no GPU: the program's host half runs everywhere"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "EVALUATE_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

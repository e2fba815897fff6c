"""Checked Shamir reconstruction on the host side: pvw_shamir_reconstruct_checked_host against a restatement of
the contract in Python integers (Lagrange interpolation through the basis columns, by pow and %), the argument errors, what one
corrupted share does to the report, agreement with pvw_shamir_reconstruct when there are no extras, and the C++ mirror.
No device compute here; the kernels are checked against the host routine in tests/test_gpu_shamir_check.py.

The grid: t in {0, 1, 2, 5}, count from t + 1 to t + 6, S in {1, 3}, both layouts, unsorted and non-contiguous indices with one
near 2^40, unreduced words (share + p), p in {257, 2^61 - 1, 2^62 - 57}."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS = 1
U64 = (1 << 64) - 1
P61 = (1 << 61) - 1
P62 = (1 << 62) - 57
PRIMES = (257, P61, P62)
NEW = ["pvw_shamir_reconstruct_checked_host", "pvw_shamir_reconstruct_checked_device", "pvw_shamir_reconstruct_checked"]


def restated(indices, rows, t, p):
    """rows [S][count] of Python integers (any words) -> (out, bad, col_bad): F_s through columns 0..t by Lagrange
    interpolation, evaluated at 0 and at the point of every other column"""
    xs = [i + 1 for i in indices]
    count = len(xs)

    def interpolate(row, x):
        total = 0
        for j in range(t + 1):
            num = den = 1
            for i in range(t + 1):
                if i != j:
                    num = num * (x - xs[i]) % p
                    den = den * (xs[j] - xs[i]) % p
            total += (row[j] % p) * num * pow(den, p - 2, p)
        return total % p

    out, bad, col_bad = [], [], [0] * count
    for row in rows:
        out.append(interpolate(row, 0))
        off = [c for c in range(t + 1, count) if row[c] % p != interpolate(row, xs[c])]
        bad.append(len(off))
        for c in off:
            col_bad[c] += 1
    return out, bad, col_bad


def indices_for(count, p, rng):
    """distinct, unsorted, non-contiguous; one near 2^40 where p allows it"""
    top = p - 1
    idx = set()
    if top > (1 << 41):
        idx.add((1 << 40) - 3)
    while len(idx) < count:
        idx.add(rng.randrange(min(top, 1 << 20) if top > 300 else top))
    idx = list(idx)
    rng.shuffle(idx)
    return idx


def sharing(indices, t, p, S, rng):
    """S polynomials of degree t and their values at the points: (secrets, rows [S][count])"""
    polys = [[rng.randrange(p) for _ in range(t + 1)] for _ in range(S)]
    rows = [[sum(a[j] * pow(i + 1, j, p) for j in range(t + 1)) % p for i in indices] for a in polys]
    return [a[0] for a in polys], rows


def checked_host(indices, rows, t, p, layout):
    """through the Python mirror, rows given secret-major and handed over in `layout`"""
    arr = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    out, bad, col_bad = P.shamir_reconstruct_checked(None, indices, arr, t, p, host=True, layout=layout)
    return out, bad.tolist(), col_bad.tolist()


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("t", [0, 1, 2, 5])
def test_host_equals_the_restatement(t, p):
    rng = random.Random(100 * t + p % 97)
    for count in range(t + 1, t + 7):
        for S in (1, 3):
            idx = indices_for(count, p, rng)
            secrets, rows = sharing(idx, t, p, S, rng)
            # a clean sharing, then arbitrary words in every column (unreduced: share + p where it fits a word, any 64-bit word)
            noisy = [[v + p if rng.random() < 0.5 and v + p <= U64 else v for v in row] for row in rows]
            junk = [[rng.getrandbits(64) for _ in row] for row in rows]
            for layout in ("secret_major", "party_major"):
                got = checked_host(idx, noisy, t, p, layout)
                assert got == (secrets, [0] * S, [0] * count), (t, p, count, S, layout)
                assert got == restated(idx, noisy, t, p)
                assert checked_host(idx, junk, t, p, layout) == restated(idx, junk, t, p), (t, p, count, S, layout)


@pytest.mark.parametrize("p", PRIMES)
def test_one_corrupted_extra_is_flagged_at_exactly_that_place(p):
    rng = random.Random(p % 1000)
    t, count, S = 2, 7, 3
    idx = indices_for(count, p, rng)
    secrets, rows = sharing(idx, t, p, S, rng)
    for s in range(S):
        for c in range(t + 1, count):
            bent = [list(r) for r in rows]
            bent[s][c] = (bent[s][c] + 1 + rng.randrange(p - 1)) % p
            for layout in ("secret_major", "party_major"):
                out, bad, col_bad = checked_host(idx, bent, t, p, layout)
                assert out == secrets
                assert bad == [int(i == s) for i in range(S)]
                assert col_bad == [int(i == c) for i in range(count)]


@pytest.mark.parametrize("p", PRIMES)
def test_one_corrupted_basis_share_flags_every_extra_of_its_secret(p):
    rng = random.Random(p % 999)
    t, count, S = 2, 7, 3
    idx = indices_for(count, p, rng)
    secrets, rows = sharing(idx, t, p, S, rng)
    for s in range(S):
        for c in range(t + 1):
            bent = [list(r) for r in rows]
            bent[s][c] = (bent[s][c] + 1 + rng.randrange(p - 1)) % p
            out, bad, col_bad = checked_host(idx, bent, t, p, "secret_major")
            assert out[s] != secrets[s] and [o for i, o in enumerate(out) if i != s] == [o for i, o in enumerate(secrets) if i != s]
            assert bad == [(count - t - 1) * int(i == s) for i in range(S)]
            assert col_bad == [0] * (t + 1) + [1] * (count - t - 1)
            assert (out, bad, col_bad) == restated(idx, bent, t, p)


def test_without_extras_the_result_is_that_of_the_unchecked_routine():
    rng = random.Random(9)
    for p in PRIMES:
        for t in (0, 1, 5):
            idx = indices_for(t + 1, p, rng)
            rows = [[rng.getrandbits(64) for _ in idx] for _ in range(4)]
            out, bad, col_bad = checked_host(idx, rows, t, p, "secret_major")
            assert out == P.shamir_reconstruct(idx, rows, p)
            assert bad == [0] * 4 and col_bad == [0] * (t + 1)


def _rc(p=P61, t=2, idx=(0, 7, 3, 999, 12), S=2, ss=None, ps=1, shares=True, out=True, indices=True, name="host", ctx=None):
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ix = np.array(idx, dtype=np.uint64)
    count = len(ix)
    sh = np.arange(max(1, S * max(count, 1)), dtype=np.uint64)
    o = np.full(max(S, 1), 77, dtype=np.uint64)
    bad = np.full(max(S, 1), 77, dtype=np.uint32)
    col = np.full(max(count, 1), 77, dtype=np.uint32)
    args = [p, t, ptr(ix) if indices else None, count, ptr(sh) if shares else None, S, count if ss is None else ss, ps,
            ptr(o) if out else None, ptr(bad), ptr(col)]
    if name == "host":
        rc = lib.pvw_shamir_reconstruct_checked_host(*args)
    elif name == "buffers":
        rc = lib.pvw_shamir_reconstruct_checked(ctx, *args)
    else:
        rc = lib.pvw_shamir_reconstruct_checked_device(ctx, *args, None)
    if rc != 0:
        assert (o == 77).all() and (bad == 77).all() and (col == 77).all(), "a refused call writes nothing"
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
    # bad and col_bad are optional
    lib = _ffi.lib()
    ix, sh, o = np.array([4, 1, 9], dtype=np.uint64), np.array([5, 5, 5], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pvw_shamir_reconstruct_checked_host(P61, 0, ptr(ix), 3, ptr(sh), 1, 3, 1, ptr(o), None, None) == 0 and o[0] == 5


def test_device_entry_points_refuse_the_same_arguments_before_any_device_work():
    """no GPU is needed to be refused"""
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    for name in ("buffers", "device"):
        for kw in REJECTED:
            assert _rc(name=name, ctx=prm._h, **kw) == INVALID_PARAMETERS, (name, kw)
        assert _rc(name=name, ctx=None) == INVALID_PARAMETERS


def test_device_forms_refuse_2_31_secrets_before_any_device_work():
    """the kernels' 32-bit counts: refused before the shares are read (the array behind the count holds two rows).  count >= 2^31
    cannot be reached with a real index array; the bound is one comparison beside the num_secrets one"""
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    ix, sh, o = np.arange(4, dtype=np.uint64), np.ones(8, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    for name, tail in (("pvw_shamir_reconstruct_checked_device", (None,)), ("pvw_shamir_reconstruct_checked", ())):
        rc = getattr(lib, name)(prm._h, P61, 1, ptr(ix), 4, ptr(sh), 1 << 31, 4, 1, ptr(o), None, None, *tail)
        assert rc == INVALID_PARAMETERS and "2^31" in _ffi.last_error(lib), name
    assert not o.any()


# ---- C++ mirror -------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "reconstruct_checked.cpp")
EXE = os.path.join(ROOT, "build", "reconstruct_checked_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_reconstructs_and_reports_on_the_host():
    """pvw_host::shamir_reconstruct_checked(host = true) needs no GPU: the program's host half runs everywhere"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RECONSTRUCT_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

"""Shamir reconstruction with erasures over a prime field of up to 256 bits, the CPU half:
pvw_shamir_reconstruct_wide_erasures_host against the contract restated in Python's integers (exhaustive search over all bases of
the sub-row of the columns that are not erased); small primes, where far rows decode to polynomials nobody dealt; agreement with
the wide corrected call (NULL and all-zero masks), with the one-word erasures call and with an err_mask fed back;
pvw_shamir_wide_erasure_mask_host against numpy; the refusals of all five entry points, which are made before any device work;
the names; the C++ mirror; and the kernels' erasure locator, in-place Forney pass, bounded recurrence, errata locator and finish
rule restated sequentially over pvw_wide.h, under the sanitizers, against Berlekamp-Welch on the sub-row.  No device is used."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from test_shamir_wide_host import COMPOSITE_255, PRIMES, SECP_N, W256, params
from test_shamir_wide_checked_host import CHECKED_PRIMES, PID, indices_for, sharing
from test_shamir_wide_corrected_host import oracle_row, spoil, unreduced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")
UNDECODABLE = P.SHAMIR_UNDECODABLE
RECON = ("pvw_shamir_reconstruct_wide_erasures_host", "pvw_shamir_reconstruct_wide_erasures_device",
         "pvw_shamir_reconstruct_wide_erasures")
MASKS = ("pvw_shamir_wide_erasure_mask_host", "pvw_shamir_wide_erasure_mask_device")
JUNK = (W256, 0, SECP_N, 1 << 255, 0x0123456789ABCDEF << 64)


def contract_row(xs, row, erased, t, p):
    """The contract for one row: the wide corrected contract on the sub-row of the columns that are not erased, with the same t,
    its wrong columns mapped back.  (secret, nerr, wrong columns); eps > r is undecodable."""
    cols = [c for c in range(len(xs)) if not erased[c]]
    if len(cols) < t + 1:
        return 0, UNDECODABLE, []
    got = oracle_row([xs[c] for c in cols], [row[c] for c in cols], t, p)
    if got is None:
        return 0, UNDECODABLE, []
    return got[0], len(got[1]), [cols[i] for i in got[1]]


def contract(indices, rows, erased, t, p):
    xs = [i + 1 for i in indices]
    out, nerr, col_err, bits = [], [], [0] * len(xs), set()
    for s, row in enumerate(rows):
        sec, ne, wrong = contract_row(xs, row, erased[s], t, p)
        out.append(sec)
        nerr.append(ne)
        for c in wrong:
            col_err[c] += 1
            bits.add((s, c))
    return out, nerr, col_err, bits


def pack(erased, count, padding=False):
    """packed words [S][W] of a boolean matrix [S][count]; padding: the bits at columns >= count set"""
    W = (count + 63) // 64
    m = np.zeros((len(erased), W), dtype=np.uint64)
    for s, row in enumerate(erased):
        for c, e in enumerate(row):
            if e:
                m[s][c // 64] |= np.uint64(1 << (c % 64))
        if padding and count % 64:
            m[s][W - 1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (count % 64)) - 1))
    return m


def erasures(indices, rows, erased, t, p, layout="secret_major", packed=False, padding=False):
    S, count = len(rows), len(indices)
    sh = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    if packed:
        er = pack(erased, count, padding)
    else:
        er = erased if layout == "secret_major" else [list(col) for col in zip(*erased)]
    out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, indices, sh, t, p, host=True, layout=layout, erased=er)
    assert mask.shape == (S, (count + 63) // 64)
    bits = {(s, c) for s in range(S) for c in range(64 * mask.shape[1]) if (int(mask[s][c // 64]) >> (c % 64)) & 1}
    return out, nerr.tolist(), col_err.tolist(), bits


def plans_for(rng, count, r):
    """(erased columns, overwritten columns) for every eps in {0, 1, r - 1, r, r + 1} x nu in {0, E_s, E_s + 1} that fits"""
    plans = []
    for eps in sorted({e for e in (0, 1, r - 1, r, r + 1) if 0 <= e <= count}):
        Es = (r - eps) // 2 if eps <= r else 0
        for nu in sorted({0, Es, Es + 1}):
            if eps + nu > count:
                continue
            cols = rng.sample(range(count), eps + nu)
            plans.append((cols[:eps], cols[eps:]))
    return plans


@pytest.mark.parametrize("p", CHECKED_PRIMES, ids=PID)
def test_host_form_equals_the_contract_by_exhaustive_search(p):
    """t in {0, 1, 2, 5} x r = 0..6; every row with its own mask and error set: eps in {0, 1, r - 1, r, r + 1} x nu in
    {0, E_s, E_s + 1}; both layouts, packed masks (padding bits set) and boolean ones; every second word unreduced; junk, 2^256 - 1
    included, at the erased positions.  The oracle decides what each row is; what was planted is asserted too where the contract
    fixes it (eps <= r and nu <= E_s: the planted secret, exactly the planted columns)."""
    rng = random.Random(21 + (p & 0xFFFF))
    for t in (0, 1, 2, 5):
        for r in range(7):
            count = t + 1 + r
            idx = indices_for(rng, count, p)
            plans = plans_for(rng, count, r)
            S = len(plans)
            secrets, clean = sharing(rng, idx, S, t, p)
            rows, erased = [], []
            for s, (ers, errs) in enumerate(plans):
                row = spoil(rng, clean[s], errs, p)
                row = [unreduced(rng, v, p) if (s + c) % 2 else v for c, v in enumerate(row)]
                for k, c in enumerate(ers):
                    row[c] = JUNK[(s + k) % len(JUNK)]
                rows.append(row)
                erased.append([c in ers for c in range(count)])
            want = contract(idx, rows, erased, t, p)
            for s, (ers, errs) in enumerate(plans):
                if len(ers) <= r and len(errs) <= (r - len(ers)) // 2:
                    assert want[0][s] == secrets[s] and want[1][s] == len(errs), ("planted", t, r, s)
                    assert {c for (ss, c) in want[3] if ss == s} == set(errs), ("planted bits", t, r, s)
                if len(ers) > r:
                    assert want[1][s] == UNDECODABLE, ("eps > r", t, r, s)
            assert not any(erased[s][c] for (s, c) in want[3])
            for layout in ("secret_major", "party_major"):
                for packed in (False, True):
                    got = erasures(idx, rows, erased, t, p, layout, packed, padding=packed)
                    assert got == want, (t, r, layout, packed)
            # other junk at the erased positions changes nothing
            other = [[W256 - 1 - c if erased[s][c] else v for c, v in enumerate(row)] for s, row in enumerate(rows)]
            assert erasures(idx, other, erased, t, p) == want, ("junk", t, r)
            # S = 1, row by row: col_err is the row's own
            for s in range(0, S, 3):
                one = contract(idx, [rows[s]], [erased[s]], t, p)
                assert erasures(idx, [rows[s]], [erased[s]], t, p, packed=True) == one, ("S=1", t, r, s)


@pytest.mark.parametrize("p", (65537, 257))
def test_arbitrary_words_over_a_small_prime(p):
    """far rows decode to polynomials nobody dealt: the host form must find them as the search does"""
    rng = random.Random(p)
    decoded = 0
    for t, count in ((0, 3), (1, 5), (2, 6), (1, 7)):
        idx = indices_for(rng, count, p)
        r = count - t - 1
        rows = [[rng.randrange(1 << 256) for _ in range(count)] for _ in range(12)]
        erased = [[c in rng.sample(range(count), s % (r + 2)) for c in range(count)] for s in range(12)]
        want = contract(idx, rows, erased, t, p)
        assert erasures(idx, rows, erased, t, p, packed=True) == want, (t, count)
        assert erasures(idx, rows, erased, t, p, "party_major") == want, (t, count)
        decoded += sum(n != UNDECODABLE for n in want[1])
    assert decoded > 0


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_null_and_zero_masks_are_the_wide_corrected_call_and_an_err_mask_feeds_back():
    rng = random.Random(5)
    for p in (SECP_N, 2**255 - 19):
        for t, count in ((2, 9), (0, 4), (3, 70)):
            idx = indices_for(rng, count, p)
            E = (count - t - 1) // 2
            E = min(E, 3)
            secrets, rows = sharing(rng, idx, 3, t, p)
            rows[0] = spoil(rng, rows[0], rng.sample(range(count), E), p)
            rows[1] = spoil(rng, rows[1], rng.sample(range(count), 1), p)
            base = P.shamir_reconstruct_wide_corrected(None, idx, rows, t, p, host=True)
            zero = np.zeros((3, (count + 63) // 64), dtype=np.uint64)
            assert same(P.shamir_reconstruct_wide_corrected(None, idx, rows, t, p, host=True, erased=zero), base)
            # the C entry point with erased == NULL
            lib = _ffi.lib()
            sh = api._wide([v for row in rows for v in row]).reshape(3, count, 4)
            out = np.zeros((3, 4), dtype=np.uint64)
            nerr, col, mask = np.zeros(3, dtype=np.uint32), np.zeros(count, dtype=np.uint32), np.zeros_like(zero)
            ix = np.array(idx, dtype=np.uint64)
            assert lib.pvw_shamir_reconstruct_wide_erasures_host(_ptr(api._wide_modulus(p)), t, _ptr(ix), count, _ptr(sh), 3, count, 1, None,
                                                                 _ptr(out), _ptr(nerr), _ptr(col), _ptr(mask)) == 0
            assert same((api._wide_ints(out), nerr, col, mask), base)
            # the err_mask as erased: the same secrets, no error left
            again = P.shamir_reconstruct_wide_corrected(None, idx, rows, t, p, host=True, erased=base[3])
            assert again[0] == secrets and not again[1].any() and not again[2].any() and not again[3].any()


def test_agrees_with_the_one_word_erasures_call_on_a_one_word_prime():
    rng = random.Random(13)
    for p in (65537, 2**61 - 1):
        for t, count in ((3, 9), (0, 4), (2, 3), (1, 8)):
            idx = indices_for(rng, count, p)
            r = count - t - 1
            _, rows = sharing(rng, idx, 4, t, p)
            rows[0] = spoil(rng, rows[0], rng.sample(range(count), r // 2), p)
            rows[1] = spoil(rng, rows[1], rng.sample(range(count), r // 2 + 1), p)
            rows[2] = [rng.randrange(p) for _ in range(count)]
            erased = [[c in rng.sample(range(count), s % (r + 2)) for c in range(count)] for s in range(4)]
            for layout in ("secret_major", "party_major"):
                sh = rows if layout == "secret_major" else [list(c) for c in zip(*rows)]
                er = erased if layout == "secret_major" else [list(c) for c in zip(*erased)]
                a = P.shamir_reconstruct_corrected(None, idx, sh, t, p, host=True, layout=layout, erased=er)
                b = P.shamir_reconstruct_wide_corrected(None, idx, sh, t, p, host=True, layout=layout, erased=er)
                assert same(a, b), (p, t, count, layout)


def numpy_mask(st, nz, bits, bound, S, count, NL, strides):
    ss, ps, ls = strides
    m = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
    for s in range(S):
        for c in range(count):
            offs = s * ss + c * ps + ls * np.arange(NL)
            e = False
            if st is not None:
                e = e or bool((st.reshape(-1)[offs] & np.uint32(bits)).any())
            if nz is not None:
                e = e or bool((nz.reshape(-1)[offs] > np.uint64(bound)).any())
            if e:
                m[s][c // 64] |= np.uint64(1 << (c % 64))
    return m


@pytest.mark.parametrize("NL", (1, 5, 16))
def test_mask_builder_against_numpy(NL):
    """counts either side of 64; the stride sets: limbs innermost secret-major (count NL, NL, 1), the decrypt-all report
    [party][dealer NL + w] (NL, S NL, 1), limb planes (count, 1, S count); num_limbs = 1 against the one-word builder"""
    lib = _ffi.lib()
    rng = np.random.default_rng(NL)
    for count in (1, 63, 64, 65, 130):
        S = 3
        n = S * count * NL
        st = (rng.integers(0, 16, n, dtype=np.uint32) * (rng.random(n) < 0.1)).astype(np.uint32)
        nz = rng.integers(0, 1000, n, dtype=np.uint64)
        nz[rng.random(n) < 0.02] = np.uint64(2**64 - 1)
        for strides in ((count * NL, NL, 1), (NL, S * NL, 1), (count, 1, S * count)):
            for a, b in ((st, nz), (st, None), (None, nz)):
                for bits, bound in ((0xFFFFFFFF, 998), (4, 2**64 - 1), (0, 500)):
                    want = numpy_mask(a, b, bits, bound, S, count, NL, strides)
                    got = np.full_like(want, 0xAAAAAAAAAAAAAAAA)
                    rc = lib.pvw_shamir_wide_erasure_mask_host(_ptr(a), _ptr(b), bits, bound, count, S, strides[0], strides[1], NL,
                                                               strides[2], _ptr(got))
                    assert rc == 0 and np.array_equal(got, want), (count, strides, bits, bound)
                    if NL == 1:
                        one = np.full_like(want, 0x5555555555555555)
                        assert lib.pvw_shamir_erasure_mask_host(_ptr(a), _ptr(b), bits, bound, count, S, strides[0], strides[1],
                                                                _ptr(one)) == 0
                        assert np.array_equal(one, got), (count, strides)
        # the Python wrapper, both layouts
        st2, nz2 = st.reshape(S, count * NL), nz.reshape(S, count * NL)
        got = P.shamir_wide_erasure_mask(st2, nz2, num_limbs=NL, status_bits=4, noise_bound=998, host=True)
        assert np.array_equal(got, numpy_mask(st, nz, 4, 998, S, count, NL, (count * NL, NL, 1)))
        stp, nzp = st.reshape(count, S * NL), nz.reshape(count, S * NL)
        got = P.shamir_wide_erasure_mask(stp, nzp, num_limbs=NL, status_bits=4, noise_bound=998, host=True, layout="party_major")
        assert np.array_equal(got, numpy_mask(st, nz, 4, 998, S, count, NL, (NL, S * NL, 1)))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_refusals_of_the_reconstruction_entry_points():
    """every refusal of the wide corrected forms, with a mask, made before any device work (the device entry points are called
    here without a GPU); nothing is written"""
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    count, t, S = 5, 2, 3
    idx = np.arange(count, dtype=np.uint64)
    sh = np.ones((S, count, 4), dtype=np.uint64)
    er = np.zeros((S, 1), dtype=np.uint64)
    out = np.full((S, 4), 7, dtype=np.uint64)
    nerr, col, mask = np.full(S, 7, dtype=np.uint32), np.full(count, 7, dtype=np.uint32), np.full((S, 1), 7, dtype=np.uint64)

    def call(name, pm_=pm, t_=t, idx_=idx, count_=count, sh_=sh, S_=S, ss=count, ps=1, out_=out, ctx=True, er_=er):
        args = [_ptr(pm_), t_, _ptr(idx_), count_, _ptr(sh_), S_, ss, ps, _ptr(er_), _ptr(out_), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h if ctx else None] + args
        if name.endswith("_device"):
            args.append(None)
        return getattr(lib, name)(*args)

    w = lambda v: api._wide_modulus(v)
    dup = np.array([0, 1, 2, 1, 4], dtype=np.uint64)
    for name in RECON:
        for er_ in (er, None):                                  # with a mask, and handed over to the corrected call
            assert call(name, pm_=None, er_=er_) == 1 and call(name, idx_=None, er_=er_) == 1, name
            assert call(name, sh_=None, er_=er_) == 1 and call(name, out_=None, er_=er_) == 1, name
            assert call(name, S_=0, er_=er_) == 1, name
            assert call(name, count_=t, er_=er_) == 1 and call(name, t_=count, er_=er_) == 1, name
            assert call(name, idx_=dup, er_=er_) == 1 and "duplicate" in _ffi.last_error(lib), name
            assert call(name, pm_=w(5), idx_=np.array([0, 1, 2, 3, 4], dtype=np.uint64), er_=er_) == 1, name
            assert call(name, pm_=w(2**64 - 59), idx_=np.array([0, 1, 2, 3, 2**64 - 1], dtype=np.uint64), er_=er_) == 1, name
            for bad_p in (COMPOSITE_255, SECP_N - 1, 2**256 - 190, 561, 1, 0):
                assert call(name, pm_=w(bad_p), er_=er_) == 1, (name, bad_p)
            assert call(name, ss=0, er_=er_) == 1 and "stride" in _ffi.last_error(lib), name
            assert call(name, ps=0, er_=er_) == 1, name
            if not name.endswith("_host"):
                assert call(name, ctx=False, er_=er_) == 1, name
        assert (out == 7).all() and (nerr == 7).all() and (col == 7).all() and (mask == 7).all(), name   # nothing written
    assert call(RECON[0], idx_=dup, pm_=w(561)) == 1 and "duplicate" in _ffi.last_error(lib)               # the order
    assert call(RECON[0]) == 0 and not (out == 7).all()


def test_device_forms_keep_the_bound_of_the_wide_corrected_call_with_and_without_a_mask():
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    big = 2 * 2048 + 1                                          # t = 0: r = 4096
    idx = np.arange(big, dtype=np.uint64)
    sh = np.ones((1, big, 4), dtype=np.uint64)
    er = np.zeros((1, (big + 63) // 64), dtype=np.uint64)
    out = np.full((2, 4), 7, dtype=np.uint64)
    for name, tail in ((RECON[1], (None,)), (RECON[2], ())):
        for er_ in (er, None):
            f = getattr(lib, name)
            rc = f(pr._h, _ptr(pm), 1, _ptr(idx), 4, _ptr(sh), 1 << 31, 4, 1, _ptr(er_), _ptr(out), None, None, None, *tail)
            assert rc == 1 and "2^31" in _ffi.last_error(lib), name
            rc = f(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, big, 1, _ptr(er_), _ptr(out), None, None, None, *tail)
            assert rc == 1 and "locator" in _ffi.last_error(lib) and "2048" in _ffi.last_error(lib), name
            text = _ffi.last_error(lib)
            rc = getattr(lib, name.replace("erasures", "corrected"))(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, big, 1, _ptr(out), None,
                                                                     None, None, *tail)
            assert rc == 1 and _ffi.last_error(lib) == text, name                       # the corrected call's own text
            rc = f(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, 0, 1, _ptr(er_), _ptr(out), None, None, None, *tail)
            assert rc == 1 and "stride" in _ffi.last_error(lib), name
    assert (out == 7).all()


def test_refusals_of_the_mask_builders():
    lib = _ffi.lib()
    pr = params(7)
    st = np.zeros(40, dtype=np.uint32)
    nz = np.zeros(40, dtype=np.uint64)
    out = np.full((2, 1), 7, dtype=np.uint64)

    def call(name, st_=st, nz_=nz, count=4, S=2, ss=20, ps=5, NL=5, ls=1, out_=out, ctx=True):
        args = [_ptr(st_), _ptr(nz_), 1, 1, count, S, ss, ps, NL, ls, _ptr(out_)]
        if name.endswith("_device"):
            args = [pr._h if ctx else None] + args + [None]
        return getattr(lib, name)(*args)

    for name in MASKS:
        assert call(name, st_=None, nz_=None) == 1 and call(name, out_=None) == 1, name
        assert call(name, count=0) == 1 and call(name, S=0) == 1, name
        assert call(name, ss=0) == 1 and call(name, ps=0) == 1, name
        assert call(name, NL=0) == 1 and "limbs" in _ffi.last_error(lib), name
        assert call(name, ls=0) == 1 and "stride" in _ffi.last_error(lib), name
        assert call(name, ps=0, NL=0) == 1 and "stride" in _ffi.last_error(lib), name   # the one-word builder's checks come first
    assert call(MASKS[1], ctx=False) == 1
    assert call(MASKS[1], count=1 << 31) == 1 and "2^31" in _ffi.last_error(lib)
    assert (out == 7).all()
    assert call(MASKS[0]) == 0 and not out.any()
    with pytest.raises(P.PvwError):
        P.shamir_wide_erasure_mask(None, None, num_limbs=5, host=True)
    with pytest.raises(P.PvwError):
        P.shamir_wide_erasure_mask(np.zeros((2, 7), dtype=np.uint32), None, num_limbs=5, host=True)


def test_python_wrapper_refuses_a_misshapen_mask():
    words = api._wide([5, 5, 6]).reshape(1, 3, 4)
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide_corrected(None, [4, 9, 2], words, 0, SECP_N, host=True, erased=np.zeros((1, 2), dtype=np.uint64))
    with pytest.raises(P.PvwError):
        P.shamir_reconstruct_wide_corrected(None, [4, 9, 2], words, 0, SECP_N, host=True, erased=[[True, False]])
    out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, [4, 9, 2], words, 0, SECP_N, host=True,
                                                                   erased=[[False, True, True]])
    assert out == [5] and nerr.tolist() == [0] and not col_err.any() and not mask.any()


SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_erasures_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_wide_erasures_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_names_and_cpp_mirror():
    assert "shamir_wide_erasure_mask" in P.__all__ and callable(P.shamir_wide_erasure_mask)
    for name in RECON + MASKS:
        assert name in _ffi._SIGNATURES and hasattr(_ffi.lib(), name)
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for name in RECON + MASKS:
        assert f"PVW_API int32_t {name}(" in header
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_ERASURES_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr


def test_kernel_decode_against_berlekamp_welch_under_sanitizers():
    """tests/cpp/shamir_wide_erasures.cpp: the erasure locator, the in-place Forney pass, the bounded recurrence, the errata
    locator and the finish rule in the kernels' update order and forms, sequentially, over pvw_wide.h's own product, accumulator
    and reduction, against Berlekamp-Welch by Gaussian elimination on the sub-row, on seeded rows with every (eps, nu) up to just
    beyond the bound, for each of the 13 primes.  The only sanitizer run: nothing loaded into Python is sanitized."""
    exe = os.path.join(ROOT, "build", "shamir_wide_erasures")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide_erasures.cpp"), "-o", exe])
    assert len(PRIMES) == 13
    out = subprocess.run([exe] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_ERASURES_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

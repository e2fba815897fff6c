"""Reconstruction with erasures on the host side: pvw_shamir_reconstruct_erasures_host and
pvw_shamir_evaluate_erasures_host against the contract restated in Python integers -- the exhaustive search of
_shamir_correct_util on the sub-row of the columns that are not erased, its polynomial evaluated at the targets by
_shamir_evaluate_util --, erased == NULL and an all-zero mask against the calls extended, an err_mask fed back as erased, the
mask builder against numpy, the refusals at every entry point (the device ones refuse without a GPU) and the C++ mirror.  No
device compute here; the kernels are checked against the host routines in tests/test_gpu_shamir_erasures.py.

The grid: t in {0, 1, 2, 5}, r in 0..6, S in {1, 3}, both layouts, scattered indices with one near 2^40, p in {257, 65537,
2^61 - 1, 2^62 - 57}; eps in {0, 1, r - 1, r, r + 1} with different sets per row and erasures inside the first t + 1 columns;
nu in {0, E_s, E_s + 1} errors among the rest; 2^64 - 1 at every erased position, and again with other garbage there; padding
bits set."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _shamir_correct_util import (P61, P62, U64, UNDECODABLE, bend, indices_for, mask_ints, sharing, unreduce)
from _shamir_evaluate_util import off_points, restated_values
from test_shamir_correct_host import REJECTED
from test_shamir_evaluate_host import OWN_REJECTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS = 1
PRIMES = (257, 65537, P61, P62)
NEW = ["pvw_shamir_reconstruct_erasures_host", "pvw_shamir_reconstruct_erasures_device", "pvw_shamir_reconstruct_erasures",
       "pvw_shamir_evaluate_erasures_host", "pvw_shamir_evaluate_erasures_device", "pvw_shamir_evaluate_erasures",
       "pvw_shamir_erasure_mask_host", "pvw_shamir_erasure_mask_device"]


def packed(sets, count, padding=False):
    """erased column sets, one per row -> uint64 words [S][W]; with padding, every bit at a column >= count set as well"""
    W = (count + 63) // 64
    m = np.zeros((len(sets), W), dtype=np.uint64)
    for s, cols in enumerate(sets):
        v = sum(1 << c for c in cols)
        if padding:
            v |= ((1 << (64 * W)) - 1) ^ ((1 << count) - 1)
        for k in range(W):
            m[s, k] = (v >> (64 * k)) & U64
    return m


def evaluated_host(indices, rows, t, p, targets, erased, layout="secret_major"):
    """through the Python mirror, rows given secret-major and handed over in `layout`: (values, (out, nerr, col_err, masks))"""
    arr = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    values, out, nerr, col_err, mask = P.shamir_evaluate_corrected(None, indices, arr, t, p, targets, host=True, layout=layout, erased=erased)
    return values.tolist(), (out, nerr.tolist(), col_err.tolist(), mask_ints(mask))


def corrected_host(indices, rows, t, p, erased, layout="secret_major"):
    arr = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    out, nerr, col_err, mask = P.shamir_reconstruct_corrected(None, indices, arr, t, p, host=True, layout=layout, erased=erased)
    return out, nerr.tolist(), col_err.tolist(), mask_ints(mask)


def restated_erasures(indices, rows, t, p, targets, sets):
    """the contract, literally: per row the restatement of 8.11 / 8.13 on the sub-row of the columns that are not erased, its mask
    bits and col_err scattered back to the original columns"""
    count = len(indices)
    values, out, nerr, col_err, masks = [], [], [], [0] * count, []
    for row, er in zip(rows, sets):
        keep = [c for c in range(count) if c not in er]
        v, (o, n, _, mk) = restated_values([indices[c] for c in keep], [[row[c] for c in keep]], t, p, targets)
        values.append(v[0]), out.append(o[0]), nerr.append(n[0])
        full = sum(1 << keep[i] for i in range(len(keep)) if (mk[0] >> i) & 1)
        masks.append(full)
        for c in range(count):
            col_err[c] += (full >> c) & 1
    return values, (out, nerr, col_err, masks)


def erasure_cases(t, count, r, S, rng):
    """per case one (erased set, error count) per row: eps in {0, 1, r - 1, r, r + 1}, different sets per row, nu in {0, E_s, E_s + 1};
    one case whose erasures lie inside the first t + 1 columns"""
    cols = list(range(count))
    cases = []
    for eps in sorted({0, 1, r - 1, r, r + 1}):
        if eps < 0 or eps > count:
            continue
        Es = max(r - eps, 0) // 2
        for nu in sorted({0, Es, Es + 1}):
            cases.append([(set(rng.sample(cols, eps)), nu) for _ in range(S)])
    inside = min(r, t + 1)
    if inside:
        cases.append([(set(rng.sample(cols[:t + 1], inside)), (r - inside) // 2) for _ in range(S)])
    cases.append([(set(rng.sample(cols, min((0, 1, r)[s % 3], count))), s % 2) for s in range(S)])      # another eps in every row
    return cases


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name
    assert "shamir_erasure_mask" in P.__all__ and callable(P.shamir_erasure_mask)


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("t", [0, 1, 2, 5])
def test_host_equals_the_restatement_on_the_sub_row(t, p):
    rng = random.Random(3000 * t + p % 107)
    decodable = undecodable = 0
    for r in range(0, 7):
        count = t + 1 + r
        for S in (1, 3):
            idx = indices_for(count, p, rng)
            _, rows = sharing(idx, t, p, S, rng)
            for case in erasure_cases(t, count, r, S, rng):
                bent = [list(row) for row in rows]
                sets = [er for er, _ in case]
                for s, (er, nu) in enumerate(case):
                    rest = [c for c in range(count) if c not in er]
                    bend(bent, s, rng.sample(rest, min(nu, len(rest))), p, rng)
                words = unreduce(bent, p, rng)
                junk = [list(row) for row in words]
                for s, er in enumerate(sets):
                    for c in er:
                        words[s][c] = U64
                        junk[s][c] = rng.getrandbits(64)
                targets = list(idx) + off_points(idx, p, 2, rng) + [idx[0]] if p - 1 - count >= 2 else list(idx) + [idx[0]]
                rng.shuffle(targets)
                want = restated_erasures(idx, bent, t, p, targets, sets)
                for layout in ("secret_major", "party_major"):
                    for er_arg in (packed(sets, count), packed(sets, count, padding=True),
                                   [[c in er for c in range(count)] for er in sets]):
                        if not isinstance(er_arg, np.ndarray) and layout == "party_major":
                            er_arg = [list(col) for col in zip(*er_arg)]
                        got = evaluated_host(idx, words, t, p, targets, er_arg, layout)
                        assert got == want, (t, p, r, S, case, layout)
                    assert corrected_host(idx, words, t, p, packed(sets, count), layout) == want[1]
                # the word at an erased position influences no output
                assert evaluated_host(idx, junk, t, p, targets, packed(sets, count)) == want
                for s, (er, nu) in enumerate(case):
                    if len(er) + 2 * nu <= r:
                        # within the bound the values are the DEALT shares, at erased and wrong columns as well
                        planted = [c for c in range(count) if bent[s][c] != rows[s][c]]
                        assert want[1][1][s] == len(planted) and want[1][3][s] == sum(1 << c for c in planted)
                        for j, tg in enumerate(targets):
                            if tg in idx:
                                assert want[0][s][j] == rows[s][idx.index(tg)], (t, p, r, s)
                        assert not want[1][3][s] & sum(1 << c for c in er), "an erased column is never reported as an error"
                        decodable += 1
                    elif len(er) > r:
                        assert want[1][1][s] == UNDECODABLE and want[0][s] == [0] * len(targets) and want[1][0][s] == 0
                        undecodable += 1
    assert decodable and undecodable


@pytest.mark.parametrize("p", PRIMES)
def test_arbitrary_words_also_where_a_far_row_decodes_to_another_polynomial(p):
    """rows of arbitrary 64-bit words under random masks: at p = 257 some lie within E_s of a polynomial nobody dealt"""
    rng = random.Random(p % 331)
    decoded = 0
    for t, count, S in ((0, 4, 200 if p == 257 else 12), (0, 6, 12), (1, 7, 12), (1, 8, 12), (2, 9, 12)):
        r = count - t - 1
        idx = indices_for(count, p, rng)
        rows = [[rng.getrandbits(64) for _ in idx] for _ in range(S)]
        sets = [set(rng.sample(range(count), rng.randrange(r - 1))) for _ in range(S)]      # eps <= r - 2: never plain interpolation
        targets = list(idx) + off_points(idx, p, 3, rng)
        want = restated_erasures(idx, rows, t, p, targets, sets)
        assert evaluated_host(idx, rows, t, p, targets, packed(sets, count)) == want
        decoded += sum(n != UNDECODABLE for n in want[1][1])
    if p == 257:
        assert decoded > 0
    if p > 65537:
        assert decoded == 0


@pytest.mark.parametrize("p", (65537, P61))
def test_no_mask_and_an_empty_mask_are_the_calls_extended(p):
    rng = random.Random(p % 211)
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for t, count, S in ((0, 3, 2), (2, 8, 3), (1, 70, 2)):
        idx = indices_for(count, p, rng)
        _, rows = sharing(idx, t, p, S, rng)
        E = (count - t - 1) // 2
        bend(rows, 0, rng.sample(range(count), E), p, rng)
        bend(rows, S - 1, rng.sample(range(count), E + 1), p, rng)
        targets = list(idx[:3]) + off_points(idx, p, 2, rng)
        base_v = P.shamir_evaluate_corrected(None, idx, rows, t, p, targets, host=True)
        base_c = P.shamir_reconstruct_corrected(None, idx, rows, t, p, host=True)
        zero = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
        got_v = P.shamir_evaluate_corrected(None, idx, rows, t, p, targets, host=True, erased=zero)
        got_c = P.shamir_reconstruct_corrected(None, idx, rows, t, p, host=True, erased=zero)
        for a, b in zip(base_v + base_c, got_v + got_c):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        # erased == NULL at the C entry points
        ix, sh, tg = np.array(idx, dtype=np.uint64), np.array(rows, dtype=np.uint64), np.array(targets, dtype=np.uint64)
        v = np.zeros((S, len(tg)), dtype=np.uint64)
        o, n, c, m = np.zeros(S, np.uint64), np.zeros(S, np.uint32), np.zeros(count, np.uint32), np.zeros_like(zero)
        assert lib.pvw_shamir_evaluate_erasures_host(p, t, ptr(ix), count, ptr(sh), S, count, 1, None, ptr(tg), len(tg), ptr(v), ptr(o), ptr(n),
                                                     ptr(c), ptr(m)) == 0
        for a, b in zip(base_v, (v, o, n, c, m)):
            assert np.array_equal(np.asarray(a, dtype=b.dtype), b)
        o[:] = 0
        assert lib.pvw_shamir_reconstruct_erasures_host(p, t, ptr(ix), count, ptr(sh), S, count, 1, None, ptr(o), ptr(n), ptr(c), ptr(m)) == 0
        for a, b in zip(base_c, (o, n, c, m)):
            assert np.array_equal(np.asarray(a, dtype=b.dtype), b)


def test_an_err_mask_fed_back_as_erased_decodes_without_errors():
    rng = random.Random(91)
    t, count, S, p = 2, 11, 4, P61                       # r = 8, E = 4
    idx = indices_for(count, p, rng)
    secrets, rows = sharing(idx, t, p, S, rng)
    for s, k in enumerate((0, 1, 4, 3)):
        bend(rows, s, rng.sample(range(count), k), p, rng)
    out, nerr, _, mask = P.shamir_reconstruct_corrected(None, idx, rows, t, p, host=True)
    assert out == secrets and nerr.tolist() == [0, 1, 4, 3]
    out2, nerr2, col2, mask2 = P.shamir_reconstruct_corrected(None, idx, rows, t, p, host=True, erased=mask)
    assert out2 == secrets and nerr2.tolist() == [0] * S and not col2.any() and not mask2.any()
    # four more wrong shares in row 2: with its four known ones erased that is 4 + 2 * 4 > r, and without the mask 8 > E
    bend(rows, 2, [c for c in range(count) if not (int(mask[2, 0]) >> c) & 1][:4], p, rng)
    assert P.shamir_reconstruct_corrected(None, idx, rows, t, p, host=True)[1][2] == UNDECODABLE
    assert P.shamir_reconstruct_corrected(None, idx, rows, t, p, host=True, erased=mask)[1][2] == UNDECODABLE


def test_r_known_bad_shares_decode_where_the_corrected_call_stops_at_half():
    rng = random.Random(92)
    t, count, S, p = 3, 12, 3, P62                       # r = 8: 8 erasures, or 4 unknown errors
    idx = indices_for(count, p, rng)
    secrets, rows = sharing(idx, t, p, S, rng)
    sets = [set(rng.sample(range(count), 8)), set(rng.sample(range(count), 5)), set(rng.sample(range(count), 6))]
    bent = [list(r) for r in rows]
    for s, er in enumerate(sets):
        bend(bent, s, sorted(er), p, rng)
    rest = [c for c in range(count) if c not in sets[2]]
    bend(bent, 2, rest[:1], p, rng)                      # 6 + 2 * 1 = r
    assert P.shamir_reconstruct_corrected(None, idx, bent, t, p, host=True)[1].tolist() == [UNDECODABLE] * 3
    values, out, nerr, col, mask = P.shamir_evaluate_corrected(None, idx, bent, t, p, idx, host=True, erased=packed(sets, count))
    assert out == secrets and nerr.tolist() == [0, 0, 1] and values.tolist() == rows
    assert mask_ints(mask) == [0, 0, 1 << rest[0]] and col.tolist() == [int(c == rest[0]) for c in range(count)]


@pytest.mark.parametrize("layout", ["secret_major", "party_major"])
def test_mask_builder_equals_numpy(layout):
    rng = np.random.default_rng(5)
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for count in (1, 63, 64, 65, 130):
        S = 3
        status = rng.integers(0, 8, size=(S, count), dtype=np.uint32)
        noise = rng.integers(0, 40, size=(S, count), dtype=np.uint64)
        noise[0, 0], status[0, 0] = 20, 0                # noise == noise_bound: not erased
        noise[S - 1, count - 1] = U64
        for use_st, use_nz in ((True, True), (True, False), (False, True)):
            flag = np.zeros((S, count), dtype=bool)
            if use_st:
                flag |= (status & 6) != 0
            if use_nz:
                flag |= noise > 20
            want = packed([set(np.flatnonzero(row).tolist()) for row in flag], count)
            st = status if layout == "secret_major" else np.ascontiguousarray(status.T)
            nz = noise if layout == "secret_major" else np.ascontiguousarray(noise.T)
            got = P.shamir_erasure_mask(st if use_st else None, nz.tolist() if use_nz else None, status_bits=6, noise_bound=20, layout=layout,
                                        host=True)
            assert np.array_equal(got, want), (count, layout, use_st, use_nz)
            assert not (int(got[0, 0]) & 1)
            # every word is written, padding bits 0, whatever the buffer held
            ss, ps = (count, 1) if layout == "secret_major" else (1, S)
            raw = np.full_like(want, U64)
            assert lib.pvw_shamir_erasure_mask_host(ptr(st) if use_st else None, ptr(nz) if use_nz else None, 6, 20, count, S, ss, ps, ptr(raw)) == 0
            assert np.array_equal(raw, want)
            # the mask is what the decode takes
            assert np.array_equal(P.api._erased_words(flag if layout == "secret_major" else flag.T, S, count, layout), want)


def test_mask_builder_refusals():
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st, nz, m = np.zeros(6, np.uint32), np.zeros(6, np.uint64), np.full(2, 77, np.uint64)
    ok = dict(status=ptr(st), noise=ptr(nz), count=3, S=2, ss=3, ps=1, mask=ptr(m))
    call = lambda k: lib.pvw_shamir_erasure_mask_host(k["status"], k["noise"], 1, 5, k["count"], k["S"], k["ss"], k["ps"], k["mask"])  # noqa: E731
    assert call(ok) == 0 and not m.any()
    m[:] = 77
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    dev = lambda k, ctx: lib.pvw_shamir_erasure_mask_device(ctx, k["status"], k["noise"], 1, 5, k["count"], k["S"], k["ss"], k["ps"], k["mask"], None)  # noqa: E731
    for bad in (dict(status=None, noise=None), dict(mask=None), dict(count=0), dict(S=0), dict(ss=0), dict(ps=0)):
        assert call({**ok, **bad}) == INVALID_PARAMETERS, bad
        assert dev({**ok, **bad}, prm._h) == INVALID_PARAMETERS, bad
    assert dev(ok, None) == INVALID_PARAMETERS
    for big in (dict(count=1 << 31), dict(S=1 << 31)):
        assert dev({**ok, **big}, prm._h) == INVALID_PARAMETERS and "2^31" in _ffi.last_error(lib)
    assert (m == 77).all(), "a refused call writes nothing"
    with pytest.raises(P.PvwError):
        P.shamir_erasure_mask(None, None, host=True)


def _rc(p=P61, t=2, idx=(0, 7, 3, 999, 12), S=2, ss=None, ps=1, shares=True, out=True, indices=True, name="host", ctx=None,
        targets=None, values=True, tgt=True, T=None, erased=True):
    """as the _rc of the corrected and evaluate tests, with the mask behind point_stride; targets=None: the reconstruct forms"""
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ix = np.array(idx, dtype=np.uint64)
    count = len(ix)
    sh = np.arange(max(1, S * max(count, 1)), dtype=np.uint64)
    er = np.zeros(max(S, 1) * ((count + 63) // 64 + 1), dtype=np.uint64)
    o = np.full(max(S, 1), 77, dtype=np.uint64)
    nerr = np.full(max(S, 1), 77, dtype=np.uint32)
    col = np.full(max(count, 1), 77, dtype=np.uint32)
    mask = np.full(max(S, 1) * ((count + 63) // 64 + 1), 77, dtype=np.uint64)
    head = [p, t, ptr(ix) if indices else None, count, ptr(sh) if shares else None, S, count if ss is None else ss, ps,
            ptr(er) if erased else None]
    if targets is None:
        v = o
        args = head + [ptr(o) if out else None, ptr(nerr), ptr(col), ptr(mask)]
        stem = "pvw_shamir_reconstruct_erasures"
    else:
        tg = np.array(targets, dtype=np.uint64)
        v = np.full(max(S, 1) * max(len(tg), 1), 77, dtype=np.uint64)
        args = head + [ptr(tg) if tgt else None, len(tg) if T is None else T, ptr(v) if (values and out) else None, ptr(o), ptr(nerr), ptr(col),
                       ptr(mask)]
        stem = "pvw_shamir_evaluate_erasures"
    if name == "host":
        rc = getattr(lib, stem + "_host")(*args)
    elif name == "buffers":
        rc = getattr(lib, stem)(ctx, *args)
    else:
        rc = getattr(lib, stem + "_device")(ctx, *args, None)
    if rc != 0:
        assert (v == 77).all() and (o == 77).all() and (nerr == 77).all() and (col == 77).all() and (mask == 77).all(), "a refused call writes nothing"
    return rc


def test_rejections_are_those_of_the_calls_extended():
    for erased in (True, False):
        assert _rc(erased=erased) == 0 and _rc(targets=(7, 5, 7), erased=erased) == 0
        for kw in REJECTED:
            assert _rc(erased=erased, **kw) == INVALID_PARAMETERS, kw
            text = _ffi.last_error(_ffi.lib())
            assert _rc(targets=(7, 5, 7), erased=erased, **kw) == INVALID_PARAMETERS, kw
            assert _ffi.last_error(_ffi.lib()) == text, "the text of the call extended"
        for kw in OWN_REJECTED:
            kw = {"targets": (7, 5, 7), **kw}
            assert _rc(erased=erased, **kw) == INVALID_PARAMETERS, kw
    # eps_s > r is a property of one row, not an argument error
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ix, sh = np.array([4, 1, 9], dtype=np.uint64), np.array([5, 5, 5, 6, 6, 6], dtype=np.uint64)
    er, o, n = np.array([0b011, 0b001], dtype=np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    assert lib.pvw_shamir_reconstruct_erasures_host(P61, 1, ptr(ix), 3, ptr(sh), 2, 3, 1, ptr(er), ptr(o), ptr(n), None, None) == 0
    assert o.tolist() == [0, 6] and n.tolist() == [UNDECODABLE, 0]


def test_device_entry_points_refuse_the_same_arguments_before_any_device_work():
    """no GPU is needed to be refused; with a mask the errata locator is bounded on the device as well (r + 1 <= 4096); without one
    the bound is the corrected call's own (r < 8192), with its text"""
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    lib = _ffi.lib()
    for name in ("buffers", "device"):
        for targets in (None, (7, 5, 7)):
            for kw in REJECTED + (OWN_REJECTED if targets else []):
                assert _rc(name=name, ctx=prm._h, **{"targets": targets, **kw}) == INVALID_PARAMETERS, (name, kw)
            assert _rc(name=name, ctx=None, targets=targets) == INVALID_PARAMETERS
            assert _rc(name=name, ctx=prm._h, targets=targets, t=0, S=1, idx=tuple(range(4097))) == INVALID_PARAMETERS         # r = 4096
            assert "erasures" in _ffi.last_error(lib) and "4096" in _ffi.last_error(lib)
            assert _rc(name=name, ctx=prm._h, targets=targets, t=0, S=1, idx=tuple(range(8193)), erased=False) == INVALID_PARAMETERS   # r = 8192
            assert "8192" in _ffi.last_error(lib) and "erasures" not in _ffi.last_error(lib)
        assert _rc(name=name, ctx=prm._h, targets=(7,), T=1 << 31) == INVALID_PARAMETERS and "num_targets" in _ffi.last_error(lib)


def test_device_forms_refuse_2_31_secrets_before_any_device_work():
    """the kernels' 32-bit counts, with a mask as without: refused before the shares are read (the arrays behind the count hold two
    rows)"""
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    prm = P.PvwParametersBuilder().set_parties(8).set_dimension(2).set_l(8).set_moduli([0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]).build()
    ix, sh, er = np.arange(4, dtype=np.uint64), np.ones(8, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    tg, v = np.array([9], dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    for tail in ((None,), ()):
        suffix = "_device" if tail else ""
        rc = getattr(lib, "pvw_shamir_reconstruct_erasures" + suffix)(prm._h, P61, 1, ptr(ix), 4, ptr(sh), 1 << 31, 4, 1, ptr(er), ptr(v), None, None,
                                                                      None, *tail)
        assert rc == INVALID_PARAMETERS and "2^31" in _ffi.last_error(lib), suffix
        rc = getattr(lib, "pvw_shamir_evaluate_erasures" + suffix)(prm._h, P61, 1, ptr(ix), 4, ptr(sh), 1 << 31, 4, 1, ptr(er), ptr(tg), 1, ptr(v),
                                                                   None, None, None, None, *tail)
        assert rc == INVALID_PARAMETERS and "2^31" in _ffi.last_error(lib) and "num_targets" not in _ffi.last_error(lib), suffix
    assert not v.any()


# ---- C++ mirror -------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "reconstruct_erasures.cpp")
EXE = os.path.join(ROOT, "build", "reconstruct_erasures_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_decodes_with_erasures_on_the_host():
    """the pvw_host overloads (host = true) need no GPU: the program's host half runs everywhere"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ERASURES_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

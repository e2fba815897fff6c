"""Wide share repair at field points, the CPU half: pvw_shamir_evaluate_wide_corrected_at_host / _erasures_at_host
against the contract restated in Python's integers -- the exhaustive search over all bases of the sub-row of the columns that are
not erased finds each row's polynomial, which is then evaluated at the points (0, 1, p - 1, p - 2, 2^64, 2^200, points on right,
wrong and erased columns, duplicates, shuffles); the point 0 against out; points = targets + 1 against the index call;
pvw_shamir_packed_wide_secrets_host against the Python definition, pvw_shamir_reconstruct_packed_wide and the older route through
corrected shares; pack = 1 against the wide erasures call; every refusal of all nine entry points, which are made before any
device work; the names; the C++ mirror; and the kernels at the new points restated sequentially over pvw_wide.h, under the
sanitizers, against Horner on the Berlekamp-Welch polynomial.  No device is used."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from test_shamir_wide_host import COMPOSITE_255, PRIMES, SECP_N, W256, params
from test_shamir_wide_checked_host import indices_for, lagrange_at, sharing
from test_shamir_wide_corrected_host import spoil, unreduced
from test_shamir_wide_erasures_host import JUNK, contract_row, pack, plans_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")
UNDECODABLE = P.SHAMIR_UNDECODABLE
P65 = 2**64 + 13
AT_PRIMES = [257, 65537, P65, 2**255 - 19, SECP_N]
PID = lambda p: f"{p.bit_length()}bit_{p & 0xFF:02x}"
AT = tuple(f"pvw_shamir_evaluate_wide_{kind}_at{form}" for kind in ("corrected", "erasures") for form in ("_host", "_device", ""))
PACKED = tuple(f"pvw_shamir_packed_wide_secrets{form}" for form in ("_host", "_device", ""))


def restated(indices, rows, erased, t, p, points):
    """The contract: (values [S][T], secrets, nerr, col_err, mask bits).  The search decides each row; the found polynomial is the
    interpolant of t + 1 columns it agrees with, evaluated at every point."""
    xs = [i + 1 for i in indices]
    values, out, nerr, col_err, bits = [], [], [], [0] * len(xs), set()
    for s, row in enumerate(rows):
        sec, ne, wrong = contract_row(xs, row, erased[s], t, p)
        out.append(sec)
        nerr.append(ne)
        if ne == UNDECODABLE:
            values.append([0] * len(points))
            continue
        for c in wrong:
            col_err[c] += 1
            bits.add((s, c))
        right = [c for c in range(len(xs)) if not erased[s][c] and c not in wrong][:t + 1]
        bx, by = [xs[c] for c in right], [row[c] % p for c in right]
        values.append([lagrange_at(bx, by, x, p) for x in points])
    return values, out, nerr, col_err, bits


def bits_of(mask, S):
    return {(s, c) for s in range(S) for c in range(64 * mask.shape[1]) if (int(mask[s][c // 64]) >> (c % 64)) & 1}


def evaluated_at(indices, rows, erased, t, p, points, layout="secret_major", packed=False):
    """the host form through the Python mirror, rows and mask given secret-major and handed over in `layout`; erased None: the
    maskless call"""
    S, count = len(rows), len(indices)
    sh = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    er = None
    if erased is not None:
        er = pack(erased, count, True) if packed else (erased if layout == "secret_major" else [list(c) for c in zip(*erased)])
    values, out, nerr, col_err, mask = P.shamir_evaluate_wide_corrected_at(None, indices, sh, t, p, points, host=True, layout=layout,
                                                                           erased=er)
    return values, out, nerr.tolist(), col_err.tolist(), bits_of(mask, S)


def evaluated(indices, rows, erased, t, p, targets):
    S = len(rows)
    er = None if erased is None else pack(erased, len(indices))
    values, out, nerr, col_err, mask = P.shamir_evaluate_wide_corrected(None, indices, rows, t, p, targets, host=True, erased=er)
    return values, out, nerr.tolist(), col_err.tolist(), bits_of(mask, S)


def point_mixes(rng, indices, wrong, erased_cols, p):
    """the point sets of the issue: the edges of the field (0, 1, p - 1, p - 2, 2^64 and 2^200 where below p), points on right,
    wrong and erased columns, all columns, duplicates, a shuffled mix with random elements"""
    count = len(indices)
    edges = [0, 1, p - 1, p - 2] + [x for x in (2**64, 2**200) if x < p]
    mixes = {"edges": edges, "zero": [0], "columns": [i + 1 for i in indices]}
    if wrong:
        mixes["wrong"] = [indices[c] + 1 for c in sorted(wrong)]
    if erased_cols:
        mixes["erased"] = [indices[c] + 1 for c in sorted(erased_cols)]
    right = [indices[c] + 1 for c in range(count) if c not in wrong and c not in erased_cols]
    if right:
        mixes["right"] = right
    mixes["duplicates"] = [0, indices[0] + 1, 0, p - 1, indices[0] + 1, p - 1]
    mixed = edges + [i + 1 for i in indices] + [rng.randrange(p) for _ in range(3)] + [indices[-1] + 1, 0]
    rng.shuffle(mixed)
    mixes["mixed"] = mixed
    return mixes


@pytest.mark.parametrize("p", AT_PRIMES, ids=PID)
def test_at_host_forms_equal_the_contract_by_exhaustive_search(p):
    """t in {0, 1, 2, 5} x r = 0..6; every row with its own mask and error set: eps in {0, 1, r - 1, r, r + 1} x nu in
    {0, E_s, E_s + 1}; both layouts, packed masks (padding bits set) and boolean ones; every second word unreduced; junk at the
    erased positions.  The value at the point 0 is out; the reports are those of the index call; points = targets + 1 is the
    index call on all five outputs."""
    rng = random.Random(25 + (p & 0xFFFF))
    seen = set()
    for t in (0, 1, 2, 5):
        for r in range(7):
            count = t + 1 + r
            idx = indices_for(rng, count, p)
            plans = plans_for(rng, count, r)
            S = len(plans)
            _, clean = sharing(rng, idx, S, t, p)
            rows, erased = [], []
            for s, (ers, errs) in enumerate(plans):
                row = spoil(rng, clean[s], errs, p)
                row = [unreduced(rng, v, p) if (s + c) % 2 else v for c, v in enumerate(row)]
                for k, c in enumerate(ers):
                    row[c] = JUNK[(s + k) % len(JUNK)]
                rows.append(row)
                erased.append([c in ers for c in range(count)])
            wrong = {c for (_, errs) in plans for c in errs}
            gone = {c for (ers, _) in plans for c in ers}
            mixes = point_mixes(rng, idx, wrong, gone, p)
            seen.update(mixes)
            none = [[False] * count for _ in rows]
            for name, points in mixes.items():
                want = restated(idx, rows, erased, t, p, points)
                for layout in ("secret_major", "party_major"):
                    got = evaluated_at(idx, rows, erased, t, p, points, layout, packed=layout == "party_major")
                    assert got == want, (t, r, name, layout)
                for j, x in enumerate(points):
                    if x == 0:
                        assert [v[j] for v in want[0]] == want[1], ("the point 0 is out", t, r, name)
                for s, (ers, errs) in enumerate(plans):
                    if len(ers) <= r and len(errs) <= (r - len(ers)) // 2:
                        for j, x in enumerate(points):
                            if x - 1 in idx:
                                assert want[0][s][j] == clean[s][idx.index(x - 1)], ("dealt", t, r, s, name)
                    if len(ers) > r:
                        assert want[0][s] == [0] * len(points) and want[2][s] == UNDECODABLE
                if name in ("mixed", "edges"):
                    assert evaluated_at(idx, rows, None, t, p, points) == restated(idx, rows, none, t, p, points), ("maskless", t, r)
            # the index call: its targets' points handed over as field elements
            targets = list(idx) + [i for i in range(min(p - 1, 300)) if i not in idx][:3] + [idx[0]]
            rng.shuffle(targets)
            for er in (erased, None):
                assert evaluated_at(idx, rows, er, t, p, [i + 1 for i in targets], packed=True) == evaluated(idx, rows, er, t, p, targets)
    assert {"edges", "zero", "columns", "wrong", "erased", "right", "duplicates", "mixed"} <= seen


def test_a_point_of_2_64_is_the_target_2_64_minus_1():
    rng = random.Random(3)
    top = 2**64 - 1
    idx = [5, 0, 77, 12]
    secrets, rows = sharing(rng, idx + [top], 2, 1, SECP_N)
    held = [row[:4] for row in rows]
    values, out, nerr, _, _ = P.shamir_evaluate_wide_corrected_at(None, idx, held, 1, SECP_N, [2**64, 6, 0], host=True)
    assert out == secrets and nerr.tolist() == [0, 0]
    assert values == [[row[4], row[0], sec] for row, sec in zip(rows, secrets)]


# ------------------------------------------------------------------------------------------------------------------ packed secrets
def packed_sharing(rng, p, S, t, K, count):
    """S packed rows over p: the coefficients of polynomials of degree t + K - 1, the shares of `count` parties whose indices are
    below p - K, and the secrets F_s(-m)"""
    def f(poly, x):
        v = 0
        for a in reversed(poly):
            v = (v * x + a) % p
        return v

    idx = rng.sample(range(min(p - K, 1 << 20)), count)
    polys = [[rng.randrange(p) for _ in range(t + K)] for _ in range(S)]
    return idx, [[f(poly, i + 1) for i in idx] for poly in polys], [[f(poly, -m) for m in range(K)] for poly in polys]


def packed_definition(indices, rows, erased, t, K, p):
    """the Python definition: the contract's decode at polynomial degree t + K - 1, then the found polynomial at the points -m"""
    values, _, nerr, col_err, bits = restated(indices, rows, erased, t + K - 1, p, [(-m) % p for m in range(K)])
    return values, nerr, col_err, bits


def packed_host(indices, rows, erased, t, K, p, layout="secret_major"):
    S = len(rows)
    sh = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    er = None if erased is None else pack(erased, len(indices), True)
    sec, nerr, col_err, mask = P.shamir_packed_wide_secrets(None, p, K, t, indices, sh, er, host=True, layout=layout)
    return sec, nerr.tolist(), col_err.tolist(), bits_of(mask, S)


@pytest.mark.parametrize("K", (1, 2, 5, 64, 65))
def test_packed_host_form_equals_the_definition_and_both_older_routes(K):
    """t in {0, 1, 3} x r in {0, 1, 2, 5}: a clean row, floor(r / 2) errors inside the first t + K columns (the basis of the older
    route) and outside them, r erasures, a mix, and a row just beyond the bound, which gives zeros.  Against the exhaustive search
    where it is affordable (K <= 5), the planted secrets, pvw_shamir_reconstruct_packed_wide on the clean row, and
    shamir_reconstruct_packed_wide_corrected(host=True) on every case."""
    rng = random.Random(2300 + K)
    for k, t in enumerate((0, 1, 3)):
        for r in (0, 1, 2, 5):
            p = (AT_PRIMES if K < 64 else [P65, 2**255 - 19, SECP_N])[(k + r) % (5 if K < 64 else 3)]
            if K >= 64 and (t, r) not in ((0, 0), (1, 2), (3, 5)):
                continue                                                                # the host form is cubic in count
            count = t + K + r
            idx, clean, secrets = packed_sharing(rng, p, 6, t, K, count)
            E = r // 2
            inside, outside = rng.sample(range(t + K), min(E, t + K)), rng.sample(range(t + K, count), min(E, r))
            eps = r - 2 * (r // 3) if r else 0
            mixed = rng.sample(range(count), eps + (r - eps) // 2)
            beyond = (rng.sample(range(count), r + 1), []) if r % 2 or r == 0 else ([], rng.sample(range(count), E + 1))
            plans = [([], []), ([], inside), ([], outside), (rng.sample(range(count), r), []), (mixed[:eps], mixed[eps:]), beyond]
            rows, erased = [], []
            for s, (ers, errs) in enumerate(plans):
                row = spoil(rng, clean[s], errs, p)
                row = [unreduced(rng, v, p) if (s + c) % 2 else v for c, v in enumerate(row)]
                for j, c in enumerate(ers):
                    row[c] = JUNK[(s + j) % len(JUNK)]
                rows.append(row)
                erased.append([c in ers for c in range(count)])
            got = packed_host(idx, rows, erased, t, K, p)
            assert got == packed_host(idx, rows, erased, t, K, p, "party_major"), (K, t, r)
            for s, (ers, errs) in enumerate(plans[:5]):
                assert got[0][s] == secrets[s] and got[1][s] == len(errs), ("planted", K, t, r, s)
                assert {c for (ss, c) in got[3] if ss == s} == set(errs), ("planted bits", K, t, r, s)
            if p > 2**60:                                                               # a far row of a small field may decode
                assert got[0][5] == [0] * K and got[1][5] == UNDECODABLE, ("beyond the bound", K, t, r)
            if K <= 5:
                assert got == packed_definition(idx, rows, erased, t, K, p), ("definition", K, t, r)
            assert got[0][0] == P.shamir_reconstruct_packed_wide(idx, [rows[0]], p, K)[0], ("the clean row", K, t, r)
            old = P.shamir_reconstruct_packed_wide_corrected(None, p, K, t, idx, rows, pack(erased, count), host=True)
            assert (old[0], old[1].tolist(), old[2].tolist(), bits_of(old[3], 6)) == got, ("the older route", K, t, r)
            none = [[False] * count for _ in rows]
            plain = packed_host(idx, rows, None, t, K, p)
            assert plain == packed_host(idx, rows, none, t, K, p), ("a zero mask", K, t, r)
            old = P.shamir_reconstruct_packed_wide_corrected(None, p, K, t, idx, rows, host=True)
            assert (old[0], old[1].tolist(), old[2].tolist(), bits_of(old[3], 6)) == plain, ("the older route, maskless", K, t, r)
            if K == 1:
                for er in (pack(erased, count), None):
                    a = P.shamir_reconstruct_wide_corrected(None, idx, rows, t, p, host=True, erased=er)
                    b = P.shamir_packed_wide_secrets(None, p, 1, t, idx, rows, er, host=True)
                    assert [[v] for v in a[0]] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), ("pack = 1", t, r)


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_refusals_of_the_six_at_entry_points():
    """what the matching index form refuses, with its text and in its order, then the points; made before any device work (the
    device entry points are called here without a GPU); nothing is written"""
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    count, t, S, T = 5, 2, 3, 2
    idx = np.arange(count, dtype=np.uint64)
    sh = np.ones((S, count, 4), dtype=np.uint64)
    er = np.zeros((S, 1), dtype=np.uint64)
    pts = api._wide([0, SECP_N - 1])
    tg = np.array([1, 9], dtype=np.uint64)
    val = np.full((S, T, 4), 7, dtype=np.uint64)
    out = np.full((S, 4), 7, dtype=np.uint64)
    nerr, col, mask = np.full(S, 7, dtype=np.uint32), np.full(count, 7, dtype=np.uint32), np.full((S, 1), 7, dtype=np.uint64)

    def call(name, pm_=pm, t_=t, idx_=idx, count_=count, sh_=sh, S_=S, ss=count, ps=1, pts_=pts, T_=T, val_=val, out_=out, ctx=True, er_=er):
        args = [_ptr(pm_), t_, _ptr(idx_), count_, _ptr(sh_), S_, ss, ps]
        if "erasures" in name:
            args.append(_ptr(er_))
        args += [_ptr(pts_), T_, _ptr(val_), _ptr(out_), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h if ctx else None] + args
        if name.endswith("_device"):
            args.append(None)
        return getattr(lib, name)(*args)

    def index_text(name, **kw):
        """the text the matching index form refuses the same arguments with"""
        other = name.replace("_at", "")
        args = [_ptr(kw.get("pm_", pm)), kw.get("t_", t), _ptr(kw.get("idx_", idx)), kw.get("count_", count), _ptr(kw.get("sh_", sh)),
                kw.get("S_", S), kw.get("ss", count), kw.get("ps", 1)]
        if "erasures" in name:
            args.append(_ptr(kw.get("er_", er)))
        args += [_ptr(tg), T, _ptr(val), _ptr(out), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h] + args
        if name.endswith("_device"):
            args.append(None)
        assert getattr(lib, other)(*args) == 1, other
        return _ffi.last_error(lib)

    w = lambda v: api._wide_modulus(v)
    dup = np.array([0, 1, 2, 1, 4], dtype=np.uint64)
    for name in AT:
        for er_ in (er, None):
            same = [dict(pm_=None), dict(idx_=None), dict(sh_=None), dict(S_=0), dict(count_=t), dict(t_=count), dict(idx_=dup),
                    dict(pm_=w(5), idx_=np.array([0, 1, 2, 3, 4], dtype=np.uint64)),
                    dict(pm_=w(2**64 - 59), idx_=np.array([0, 1, 2, 3, 2**64 - 1], dtype=np.uint64)), dict(ss=0), dict(ps=0)]
            same += [dict(pm_=w(bad)) for bad in (COMPOSITE_255, SECP_N - 1, 2**256 - 190, 561, 1, 0)]
            for kw in same:
                assert call(name, er_=er_, **kw) == 1, (name, kw)
                text = _ffi.last_error(lib)
                assert text == index_text(name, er_=er_, **kw), (name, kw)
            assert call(name, er_=er_, idx_=dup, pts_=None) == 1 and "duplicate" in _ffi.last_error(lib), name     # the order
            assert call(name, er_=er_, val_=None) == 1 and "NULL" in _ffi.last_error(lib), name
            assert call(name, er_=er_, pts_=None) == 1 and "NULL" in _ffi.last_error(lib), name
            assert call(name, er_=er_, T_=0) == 1 and "no points" in _ffi.last_error(lib), name
            for bad in (SECP_N, SECP_N + 1, W256):
                assert call(name, er_=er_, pts_=api._wide([0, bad])) == 1 and "point out of range" in _ffi.last_error(lib), (name, bad)
            assert call(name, er_=er_, pm_=w(65537), pts_=api._wide([1, 65537])) == 1 and "point out of range" in _ffi.last_error(lib), name
            if not name.endswith("_host"):
                assert call(name, ctx=False, er_=er_) == 1, name
                assert call(name, er_=er_, T_=1 << 31) == 1 and "num_points" in _ffi.last_error(lib), name       # before the walk
        assert (val == 7).all() and (out == 7).all() and (nerr == 7).all() and (col == 7).all() and (mask == 7).all(), name
    for name in (AT[0], AT[3]):
        assert call(name, out_=None) == 0 and not (val == 7).all() and (out == 7).all()                          # out may be NULL
        val[:] = 7
        assert call(name) == 0 and not (out == 7).all()
        val[:], out[:], nerr[:], col[:], mask[:] = 7, 7, 7, 7, 7
    # the device bound of the wide corrected call, with and without a mask, before the points are looked at
    big = 2 * 2048 + 1                                          # t = 0: r = 4096
    bidx = np.arange(big, dtype=np.uint64)
    bsh = np.ones((1, big, 4), dtype=np.uint64)
    ber = np.zeros((1, (big + 63) // 64), dtype=np.uint64)
    for name in (AT[1], AT[2], AT[4], AT[5]):
        for er_ in (ber, None):
            assert call(name, t_=0, idx_=bidx, count_=big, sh_=bsh, S_=1, ss=big, er_=er_, pts_=None) == 1, name
            assert "locator" in _ffi.last_error(lib) and "2048" in _ffi.last_error(lib), name
    assert (val == 7).all()


def test_refusals_of_the_three_packed_entry_points():
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    count, t, K, S = 8, 2, 3, 3
    idx = np.arange(count, dtype=np.uint64)
    sh = np.ones((S, count, 4), dtype=np.uint64)
    er = np.zeros((S, 1), dtype=np.uint64)
    sec = np.full((S, K, 4), 7, dtype=np.uint64)
    nerr, col, mask = np.full(S, 7, dtype=np.uint32), np.full(count, 7, dtype=np.uint32), np.full((S, 1), 7, dtype=np.uint64)

    def call(name, pm_=pm, K_=K, t_=t, idx_=idx, count_=count, sh_=sh, S_=S, ss=count, ps=1, er_=er, sec_=sec, ctx=True):
        args = [_ptr(pm_), K_, t_, _ptr(idx_), count_, _ptr(sh_), S_, ss, ps, _ptr(er_), _ptr(sec_), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h if ctx else None] + args
        if name.endswith("_device"):
            args.append(None)
        return getattr(lib, name)(*args)

    def erasures_text(name, **kw):
        """the text the wide erasures call refuses the same arguments with at polynomial degree t + K - 1"""
        other = name.replace("packed_wide_secrets", "reconstruct_wide_erasures")
        args = [_ptr(kw.get("pm_", pm)), t + K - 1, _ptr(kw.get("idx_", idx)), kw.get("count_", count), _ptr(kw.get("sh_", sh)),
                kw.get("S_", S), kw.get("ss", count), kw.get("ps", 1), _ptr(kw.get("er_", er)), _ptr(np.zeros((S, 4), dtype=np.uint64)),
                _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h] + args
        if name.endswith("_device"):
            args.append(None)
        assert getattr(lib, other)(*args) == 1, other
        return _ffi.last_error(lib)

    w = lambda v: api._wide_modulus(v)
    dup = np.array([0, 1, 2, 1, 4, 5, 6, 7], dtype=np.uint64)
    for name in PACKED:
        for er_ in (er, None):
            for kw in (dict(pm_=None), dict(idx_=None), dict(sh_=None), dict(sec_=None)):
                assert call(name, er_=er_, **kw) == 1 and "NULL" in _ffi.last_error(lib), (name, kw)
            assert call(name, er_=er_, K_=0) == 1 and "pack must be at least 1" in _ffi.last_error(lib), name
            assert call(name, er_=er_, K_=1025) == 1, name
            assert "PVW_WIDE_MAX_PACK" in _ffi.last_error(lib), name
            assert call(name, er_=er_, K_=0, idx_=dup) == 1 and "pack" in _ffi.last_error(lib), name             # the order
            same = [dict(S_=0), dict(count_=t + K - 1), dict(idx_=dup), dict(ss=0), dict(ps=0),
                    dict(pm_=w(2**64 - 59), idx_=np.array([0, 1, 2, 3, 4, 5, 6, 2**64 - 1], dtype=np.uint64))]
            same += [dict(pm_=w(bad)) for bad in (COMPOSITE_255, SECP_N - 1, 561, 1, 0)]
            for kw in same:
                assert call(name, er_=er_, **kw) == 1, (name, kw)
                text = _ffi.last_error(lib)
                assert text == erasures_text(name, er_=er_, **kw), (name, kw)
            assert call(name, er_=er_, count_=t + K - 1) == 1 and f"at least {t + K} shares" in _ffi.last_error(lib), name
            # an index at or above p - pack: p = 257, pack = 3: 253 is the last legal index (the secret point -2 is 255 = 254 + 1)
            top = np.array([0, 1, 2, 3, 4, 5, 6, 254], dtype=np.uint64)
            assert call(name, er_=er_, pm_=w(257), idx_=top) == 1 and "plain_modulus - pack" in _ffi.last_error(lib), name
            top[7] = 253
            if name.endswith("_host"):
                assert call(name, er_=er_, pm_=w(257), idx_=top) == 0, name
                assert not (sec == 7).all()
                sec[:], nerr[:], col[:], mask[:] = 7, 7, 7, 7
            if not name.endswith("_host"):
                assert call(name, ctx=False, er_=er_) == 1 and "NULL" in _ffi.last_error(lib), name
                assert call(name, er_=er_, S_=1 << 31) == 1 and "2^31" in _ffi.last_error(lib), name
        assert (sec == 7).all() and (nerr == 7).all() and (col == 7).all() and (mask == 7).all(), name
    # the device bound r < 4096 at polynomial degree t + pack - 1
    big = 2 * 2048 + 3                                          # t = 0, pack = 3: r = 4096
    bidx = np.arange(big, dtype=np.uint64)
    bsh = np.ones((1, big, 4), dtype=np.uint64)
    for name in PACKED[1:]:
        assert call(name, t_=0, idx_=bidx, count_=big, sh_=bsh, S_=1, ss=big, er_=None) == 1, name
        assert "locator" in _ffi.last_error(lib) and "2048" in _ffi.last_error(lib), name
    with pytest.raises(P.PvwError):
        P.shamir_packed_wide_secrets(None, SECP_N, 2, 1, [0, 1, 2], [[1, 2]], host=True)                        # the wrapper's shapes
    with pytest.raises(P.PvwError):
        P.shamir_evaluate_wide_corrected_at(None, [0, 1, 2], [[1, 2, 3]], 1, SECP_N, [-1], host=True)


# ------------------------------------------------------------------------------------------------------- names, mirror, restatement
SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_points_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_wide_points_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_names_and_cpp_mirror():
    for name in ("shamir_evaluate_wide_corrected_at", "shamir_packed_wide_secrets"):
        assert name in P.__all__ and callable(getattr(P, name))
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "pvw-hip-sys", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in AT + PACKED:
            assert name in _ffi._SIGNATURES and hasattr(lib, name), name
            assert f"PVW_API int32_t {name}(" in header
            assert f"pub fn {name}(" in block
    mirror = open(os.path.join(ROOT, "pvw_rs_amd", "host", "pvw.hpp")).read()
    shims = open(os.path.join(ROOT, "rust", "pvw", "src", "crypto.rs")).read()
    for name in ("shamir_evaluate_wide_corrected_at", "shamir_packed_wide_secrets"):
        assert f" {name}(" in mirror and f"pub fn {name}(" in shims
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_POINTS_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr


def test_kernels_at_field_points_against_horner_under_sanitizers():
    """tests/cpp/shamir_wide_points.cpp: the point kernel (m -> (p - m) R, 0 -> 0) against the words of p - m through the
    kernel-argument path; then scale / coin, the Cauchy entries, Xt, Xd, the three products and the finish rule in the kernels'
    forms (the restatement of shamir_wide_evaluate.cpp, included as it is) at the points 0, p - 1, the packed points -- through 70,
    beyond one batch of 64 -- and points on right, wrong and erased columns given as field elements, for every (eps, nu) up to
    just beyond the bound at t 0..2 x r 0..5, against Horner on the Berlekamp-Welch polynomial of the sub-row and, at 0, against
    the decode's secret; for each of the 13 primes.  The only sanitizer run: nothing loaded into Python is sanitized."""
    exe = os.path.join(ROOT, "build", "shamir_wide_points")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide_points.cpp"), "-o", exe])
    assert len(PRIMES) == 13
    out = subprocess.run([exe] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SHAMIR_WIDE_POINTS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

"""Share repair over a prime field of up to 256 bits, the CPU half: pvw_shamir_evaluate_wide_corrected_host and
pvw_shamir_evaluate_wide_erasures_host against the contract restated in Python's integers -- the exhaustive search over all bases
of the sub-row of the columns that are not erased finds each row's polynomial, which is then evaluated at the targets; the four
reports against the wide corrected / erasures calls; NULL and all-zero masks; the one-word evaluate call on one-word primes; junk
at erased positions; column and target order; a target of 2^64 - 1; every refusal of all six entry points, which are made before
any device work; the names; the C++ mirror; and the kernels' y o M, scale / coin, batched-inversion Cauchy entries, derivative
powers, three products and finish rule restated sequentially over pvw_wide.h, under the sanitizers, against Horner on the
Berlekamp-Welch polynomial.  No device is used."""
import ctypes as C
import os
import random
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
P256B = 2**256 - 189
EVAL_PRIMES = [SECP_N, P256B, 2**255 - 19, 65537, 257]          # two of 256 bits, one of 255, two small
PID = lambda p: f"{p.bit_length()}bit_{p & 0xFF:02x}"
CORRECTED = ("pvw_shamir_evaluate_wide_corrected_host", "pvw_shamir_evaluate_wide_corrected_device",
             "pvw_shamir_evaluate_wide_corrected")
ERASURES = ("pvw_shamir_evaluate_wide_erasures_host", "pvw_shamir_evaluate_wide_erasures_device",
            "pvw_shamir_evaluate_wide_erasures")


def restated(indices, rows, erased, t, p, targets):
    """The contract: (values [S][T], secrets, nerr, col_err, mask bits).  The search decides each row; the found polynomial is the
    interpolant of t + 1 columns it agrees with, evaluated at every target's point."""
    xs = [i + 1 for i in indices]
    values, out, nerr, col_err, bits = [], [], [], [0] * len(xs), set()
    for s, row in enumerate(rows):
        sec, ne, wrong = contract_row(xs, row, erased[s], t, p)
        out.append(sec)
        nerr.append(ne)
        if ne == UNDECODABLE:
            values.append([0] * len(targets))
            continue
        for c in wrong:
            col_err[c] += 1
            bits.add((s, c))
        right = [c for c in range(len(xs)) if not erased[s][c] and c not in wrong][:t + 1]
        bx, by = [xs[c] for c in right], [row[c] % p for c in right]
        assert lagrange_at(bx, by, 0, p) == sec
        values.append([lagrange_at(bx, by, tg + 1, p) for tg in targets])
    return values, out, nerr, col_err, bits


def evaluated(indices, rows, erased, t, p, targets, layout="secret_major", packed=False):
    """the host form through the Python mirror, rows and mask given secret-major and handed over in `layout`; erased None: the
    maskless call"""
    S, count = len(rows), len(indices)
    sh = rows if layout == "secret_major" else [list(col) for col in zip(*rows)]
    er = None
    if erased is not None:
        er = pack(erased, count, True) if packed else (erased if layout == "secret_major" else [list(c) for c in zip(*erased)])
    values, out, nerr, col_err, mask = P.shamir_evaluate_wide_corrected(None, indices, sh, t, p, targets, host=True, layout=layout,
                                                                        erased=er)
    bits = {(s, c) for s in range(S) for c in range(64 * mask.shape[1]) if (int(mask[s][c // 64]) >> (c % 64)) & 1}
    return values, out, nerr.tolist(), col_err.tolist(), bits


def decode_only(indices, rows, erased, t, p):
    out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, indices, rows, t, p, host=True,
                                                                   erased=None if erased is None else pack(erased, len(indices)))
    S = len(rows)
    bits = {(s, c) for s in range(S) for c in range(64 * mask.shape[1]) if (int(mask[s][c // 64]) >> (c % 64)) & 1}
    return out, nerr.tolist(), col_err.tolist(), bits


def off_points(rng, indices, p, T):
    """T indices that are no column's: the largest legal one first where it is free"""
    top = min(p - 2, 2**64 - 1)
    got = [top] if top not in indices else []
    while len(got) < T:
        i = rng.randrange(min(p - 1, 1 << 24))
        if i not in indices and i not in got:
            got.append(i)
    return got[:T]


def target_mixes(rng, indices, wrong, erased_cols, p):
    """the target sets of the issue: off the points (T = 1, 2, 7), all columns, only wrong, only erased, only right, duplicates, a
    shuffled mix"""
    count = len(indices)
    room = min(p - 1, 2**64) - count
    mixes = {f"off{T}": off_points(rng, indices, p, T) for T in (1, 2, 7) if T <= room}
    mixes["columns"] = list(indices)
    if wrong:
        mixes["wrong"] = [indices[c] for c in sorted(wrong)]
    if erased_cols:
        mixes["erased"] = [indices[c] for c in sorted(erased_cols)]
    right = [indices[c] for c in range(count) if c not in wrong and c not in erased_cols]
    if right:
        mixes["right"] = right
    mixes["duplicates"] = [indices[0], indices[0]] + (mixes.get("off1", []) * 2)
    mixed = list(indices) + mixes.get("off2", []) + [indices[-1]]
    rng.shuffle(mixed)
    mixes["mixed"] = mixed
    return mixes


@pytest.mark.parametrize("p", EVAL_PRIMES, ids=PID)
def test_host_forms_equal_the_contract_by_exhaustive_search(p):
    """t in {0, 1, 2, 5} x r = 0..6; every row with its own mask and error set: eps in {0, 1, r - 1, r, r + 1} x nu in
    {0, E_s, E_s + 1}; both layouts, packed masks (padding bits set) and boolean ones; every second word unreduced; junk, 2^256 - 1
    included, at the erased positions.  The reports are those of the decode-only host call on the same input; where the contract
    fixes it (eps <= r, nu <= E_s) the values at the columns are the DEALT shares, at wrong and erased columns too."""
    rng = random.Random(22 + (p & 0xFFFF))
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
            mixes = target_mixes(rng, idx, wrong, gone, p)
            seen.update(mixes)
            reports = decode_only(idx, rows, erased, t, p)
            for name, targets in mixes.items():
                want = restated(idx, rows, erased, t, p, targets)
                assert tuple(want[1:]) == reports, ("reports", t, r, name)
                for layout in ("secret_major", "party_major"):
                    got = evaluated(idx, rows, erased, t, p, targets, layout, packed=layout == "party_major")
                    assert got == want, (t, r, name, layout)
                for s, (ers, errs) in enumerate(plans):
                    if len(ers) <= r and len(errs) <= (r - len(ers)) // 2:
                        for j, tg in enumerate(targets):
                            if tg in idx:
                                assert want[0][s][j] == clean[s][idx.index(tg)], ("dealt", t, r, s, name)
                    if len(ers) > r:
                        assert want[0][s] == [0] * len(targets) and want[2][s] == UNDECODABLE
            # other junk at the erased positions changes nothing
            targets = mixes["mixed"]
            other = [[W256 - 1 - c if erased[s][c] else v for c, v in enumerate(row)] for s, row in enumerate(rows)]
            assert evaluated(idx, other, erased, t, p, targets) == evaluated(idx, rows, erased, t, p, targets), ("junk", t, r)
            # without a mask: the maskless contract, and the wide corrected call's reports
            none = [[False] * count for _ in rows]
            want = restated(idx, rows, none, t, p, targets)
            assert evaluated(idx, rows, None, t, p, targets) == want, ("maskless", t, r)
            assert tuple(want[1:]) == decode_only(idx, rows, None, t, p)
            assert evaluated(idx, rows, none, t, p, targets, packed=True) == want, ("zero mask", t, r)
    assert {"off1", "off2", "off7", "columns", "wrong", "erased", "right", "duplicates", "mixed"} <= seen


@pytest.mark.parametrize("p", (65537, 257))
def test_arbitrary_words_over_a_small_prime(p):
    """far rows decode to polynomials nobody dealt, whose values are returned; undecodable rows are 0"""
    rng = random.Random(p + 1)
    decoded = undecodable = 0
    for t, count in ((0, 3), (1, 5), (2, 6), (1, 7)):
        idx = indices_for(rng, count, p)
        r = count - t - 1
        rows = [[rng.randrange(1 << 256) for _ in range(count)] for _ in range(12)]
        erased = [[c in rng.sample(range(count), s % (r + 2)) for c in range(count)] for s in range(12)]
        targets = list(idx) + off_points(rng, idx, p, 3)
        rng.shuffle(targets)
        want = restated(idx, rows, erased, t, p, targets)
        assert evaluated(idx, rows, erased, t, p, targets, packed=True) == want, (t, count)
        assert evaluated(idx, rows, erased, t, p, targets, "party_major") == want, (t, count)
        none = [[False] * count for _ in rows]
        assert evaluated(idx, rows, None, t, p, targets) == restated(idx, rows, none, t, p, targets), (t, count)
        decoded += sum(n != UNDECODABLE for n in want[2])
        undecodable += sum(n == UNDECODABLE for n in want[2])
        for s, n in enumerate(want[2]):
            if n == UNDECODABLE:
                assert want[0][s] == [0] * len(targets)
    assert decoded > 0 and undecodable > 0


def test_agrees_with_the_one_word_evaluate_call_on_a_one_word_prime():
    rng = random.Random(14)
    for p in (65537, 2**61 - 1, 257):
        for t, count in ((3, 9), (0, 4), (2, 3), (1, 8)):
            idx = indices_for(rng, count, p)
            r = count - t - 1
            _, rows = sharing(rng, idx, 4, t, p)
            rows[0] = spoil(rng, rows[0], rng.sample(range(count), r // 2), p)
            rows[1] = spoil(rng, rows[1], rng.sample(range(count), r // 2 + 1), p)
            rows[2] = [rng.randrange(p) for _ in range(count)]
            erased = [[c in rng.sample(range(count), s % (r + 2)) for c in range(count)] for s in range(4)]
            targets = list(idx) + off_points(rng, idx, p, 2) + [idx[0]]
            for layout in ("secret_major", "party_major"):
                sh = rows if layout == "secret_major" else [list(c) for c in zip(*rows)]
                for er in (erased, None):
                    e = er if er is None or layout == "secret_major" else [list(c) for c in zip(*er)]
                    a = P.shamir_evaluate_corrected(None, idx, sh, t, p, targets, host=True, layout=layout, erased=e)
                    b = P.shamir_evaluate_wide_corrected(None, idx, sh, t, p, targets, host=True, layout=layout, erased=e)
                    assert a[0].tolist() == b[0] and a[1] == b[1], (p, t, count, layout)
                    assert all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:])), (p, t, count, layout)


@pytest.mark.parametrize("p", (SECP_N, 65537), ids=PID)
def test_column_order_and_target_order(p):
    rng = random.Random(31)
    t, count, S = 2, 9, 3
    idx = indices_for(rng, count, p)
    _, rows = sharing(rng, idx, S, t, p)
    rows[0] = spoil(rng, rows[0], [1, 7], p)
    rows[1] = spoil(rng, rows[1], [4], p)
    erased = [[c in (3,) for c in range(count)], [c in (0, 8) for c in range(count)], [False] * count]
    targets = list(idx) + off_points(rng, idx, p, 4)
    base = evaluated(idx, rows, erased, t, p, targets)
    perm = list(range(count))
    rng.shuffle(perm)
    got = evaluated([idx[c] for c in perm], [[row[c] for c in perm] for row in rows], [[e[c] for c in perm] for e in erased], t, p, targets)
    assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2]                      # no value changes
    assert got[3] == [base[3][c] for c in perm] and got[4] == {(s, perm.index(c)) for (s, c) in base[4]}
    order = list(range(len(targets)))
    rng.shuffle(order)
    got = evaluated(idx, rows, erased, t, p, [targets[j] for j in order])
    assert got[0] == [[v[j] for j in order] for v in base[0]] and got[1:] == base[1:]          # the columns of values permute


def test_a_target_of_2_64_minus_1_under_a_256_bit_prime_and_above_a_64_bit_one():
    rng = random.Random(3)
    top = 2**64 - 1
    idx = [5, 0, 77, 12]
    secrets, rows = sharing(rng, idx + [top], 2, 1, SECP_N)
    held = [row[:4] for row in rows]
    values, out, nerr, _, _ = P.shamir_evaluate_wide_corrected(None, idx, held, 1, SECP_N, [top, 5], host=True)
    assert out == secrets and nerr.tolist() == [0, 0]
    assert values == [[row[4], row[0]] for row in rows]
    for p in (2**64 - 59, 2**64 + 1 - 2**32):                                                # one word: the point 2^64 is not below p
        with pytest.raises(P.PvwError):
            P.shamir_evaluate_wide_corrected(None, idx, held, 1, p, [top], host=True)
    P.shamir_evaluate_wide_corrected(None, idx, held, 1, 2**64 + 13, [top], host=True)        # p > 2^64 + 1: legal


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_the_erasures_entry_point_with_a_null_mask_is_the_maskless_call():
    rng = random.Random(6)
    lib = _ffi.lib()
    for p in (SECP_N, 65537):
        t, count, S = 2, 9, 3
        idx = indices_for(rng, count, p)
        _, rows = sharing(rng, idx, S, t, p)
        rows[0] = spoil(rng, rows[0], [1, 7], p)
        rows[1] = spoil(rng, rows[1], [0, 3, 4, 8], p)
        targets = list(idx) + off_points(rng, idx, p, 3)
        base = P.shamir_evaluate_wide_corrected(None, idx, rows, t, p, targets, host=True)
        sh = api._wide([v for row in rows for v in row]).reshape(S, count, 4)
        ix, tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
        val, out = np.zeros((S, len(tg), 4), dtype=np.uint64), np.zeros((S, 4), dtype=np.uint64)
        nerr, col, mask = np.zeros(S, dtype=np.uint32), np.zeros(count, dtype=np.uint32), np.zeros((S, 1), dtype=np.uint64)
        assert lib.pvw_shamir_evaluate_wide_erasures_host(_ptr(api._wide_modulus(p)), t, _ptr(ix), count, _ptr(sh), S, count, 1, None, _ptr(tg),
                                                          len(tg), _ptr(val), _ptr(out), _ptr(nerr), _ptr(col), _ptr(mask)) == 0
        assert [api._wide_ints(v) for v in val] == base[0] and api._wide_ints(out) == base[1]
        assert np.array_equal(nerr, base[2]) and np.array_equal(col, base[3]) and np.array_equal(mask, base[4])
        assert base[2].tolist()[:2] == [2, P.SHAMIR_UNDECODABLE] and base[0][1] == [0] * len(targets)


def test_refusals_of_all_six_entry_points():
    """what the matching wide corrected / erasures form refuses, with its text and in its order, then the targets; made before any
    device work (the device entry points are called here without a GPU); nothing is written"""
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    count, t, S, T = 5, 2, 3, 2
    idx = np.arange(count, dtype=np.uint64)
    sh = np.ones((S, count, 4), dtype=np.uint64)
    er = np.zeros((S, 1), dtype=np.uint64)
    tg = np.array([1, 9], dtype=np.uint64)
    val = np.full((S, T, 4), 7, dtype=np.uint64)
    out = np.full((S, 4), 7, dtype=np.uint64)
    nerr, col, mask = np.full(S, 7, dtype=np.uint32), np.full(count, 7, dtype=np.uint32), np.full((S, 1), 7, dtype=np.uint64)

    def call(name, pm_=pm, t_=t, idx_=idx, count_=count, sh_=sh, S_=S, ss=count, ps=1, tg_=tg, T_=T, val_=val, out_=out, ctx=True, er_=er):
        args = [_ptr(pm_), t_, _ptr(idx_), count_, _ptr(sh_), S_, ss, ps]
        if "erasures" in name:
            args.append(_ptr(er_))
        args += [_ptr(tg_), T_, _ptr(val_), _ptr(out_), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h if ctx else None] + args
        if name.endswith("_device"):
            args.append(None)
        return getattr(lib, name)(*args)

    def decode_text(name, **kw):
        """the text the matching decode-only form refuses the same arguments with"""
        other = name.replace("evaluate", "reconstruct")
        args = [_ptr(kw.get("pm_", pm)), kw.get("t_", t), _ptr(kw.get("idx_", idx)), kw.get("count_", count), _ptr(kw.get("sh_", sh)),
                kw.get("S_", S), kw.get("ss", count), kw.get("ps", 1)]
        if "erasures" in name:
            args.append(_ptr(kw.get("er_", er)))
        args += [_ptr(out), _ptr(nerr), _ptr(col), _ptr(mask)]
        if not name.endswith("_host"):
            args = [pr._h] + args
        if name.endswith("_device"):
            args.append(None)
        assert getattr(lib, other)(*args) == 1, other
        return _ffi.last_error(lib)

    w = lambda v: api._wide_modulus(v)
    dup = np.array([0, 1, 2, 1, 4], dtype=np.uint64)
    for name in CORRECTED + ERASURES:
        for er_ in (er, None):
            same = [dict(pm_=None), dict(idx_=None), dict(sh_=None), dict(S_=0), dict(count_=t), dict(t_=count), dict(idx_=dup),
                    dict(pm_=w(5), idx_=np.array([0, 1, 2, 3, 4], dtype=np.uint64)),
                    dict(pm_=w(2**64 - 59), idx_=np.array([0, 1, 2, 3, 2**64 - 1], dtype=np.uint64)), dict(ss=0), dict(ps=0)]
            same += [dict(pm_=w(bad)) for bad in (COMPOSITE_255, SECP_N - 1, 2**256 - 190, 561, 1, 0)]
            for kw in same:
                assert call(name, er_=er_, **kw) == 1, (name, kw)
                text = _ffi.last_error(lib)
                assert text == decode_text(name, er_=er_, **kw), (name, kw)
            assert call(name, er_=er_, idx_=dup, tg_=None) == 1 and "duplicate" in _ffi.last_error(lib), name     # the order
            assert call(name, er_=er_, val_=None) == 1 and "NULL" in _ffi.last_error(lib), name
            assert call(name, er_=er_, tg_=None) == 1 and "NULL" in _ffi.last_error(lib), name
            assert call(name, er_=er_, T_=0) == 1 and "no targets" in _ffi.last_error(lib), name
            assert call(name, er_=er_, pm_=w(65537), tg_=np.array([1, 65536], dtype=np.uint64)) == 1, name
            assert "target index out of range" in _ffi.last_error(lib), name
            assert call(name, er_=er_, pm_=w(2**64 - 59), tg_=np.array([1, 2**64 - 1], dtype=np.uint64)) == 1, name
            if not name.endswith("_host"):
                assert call(name, ctx=False, er_=er_) == 1, name
                assert call(name, er_=er_, T_=1 << 31) == 1 and "num_targets" in _ffi.last_error(lib), name  # before the walk
        assert (val == 7).all() and (out == 7).all() and (nerr == 7).all() and (col == 7).all() and (mask == 7).all(), name
    for name in (CORRECTED[0], ERASURES[0]):
        assert call(name, out_=None) == 0 and not (val == 7).all() and (out == 7).all()                          # out may be NULL
        val[:] = 7
        assert call(name) == 0 and not (out == 7).all()
        out[:] = 7


def test_device_forms_keep_the_bound_of_the_wide_corrected_call_with_and_without_a_mask():
    lib = _ffi.lib()
    pr = params(7)
    pm = api._wide_modulus(SECP_N)
    big = 2 * 2048 + 1                                          # t = 0: r = 4096
    idx = np.arange(big, dtype=np.uint64)
    sh = np.ones((1, big, 4), dtype=np.uint64)
    er = np.zeros((1, (big + 63) // 64), dtype=np.uint64)
    tg = np.array([3], dtype=np.uint64)
    val = np.full((2, 4), 7, dtype=np.uint64)
    for k, tail in ((1, (None,)), (2, ())):
        for er_ in (er, None):
            f = getattr(lib, ERASURES[k])
            rc = f(pr._h, _ptr(pm), 1, _ptr(idx), 4, _ptr(sh), 1 << 31, 4, 1, _ptr(er_), _ptr(tg), 1, _ptr(val), None, None, None, None, *tail)
            assert rc == 1 and "2^31" in _ffi.last_error(lib)
            rc = f(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, big, 1, _ptr(er_), None, 1, _ptr(val), None, None, None, None, *tail)
            assert rc == 1 and "locator" in _ffi.last_error(lib) and "2048" in _ffi.last_error(lib)               # before the targets
            text = _ffi.last_error(lib)
            rc = getattr(lib, CORRECTED[k])(pr._h, _ptr(pm), 0, _ptr(idx), big, _ptr(sh), 1, big, 1, _ptr(tg), 1, _ptr(val), None, None, None,
                                            None, *tail)
            assert rc == 1 and _ffi.last_error(lib) == text
    assert (val == 7).all()


def test_python_wrapper_shapes():
    words = api._wide([5, 5, 6]).reshape(1, 3, 4)
    with pytest.raises(P.PvwError):
        P.shamir_evaluate_wide_corrected(None, [4, 9, 2], words, 0, SECP_N, [1], host=True, erased=np.zeros((1, 2), dtype=np.uint64))
    values, out, nerr, col_err, mask = P.shamir_evaluate_wide_corrected(None, [4, 9, 2], words, 0, SECP_N, [2, 100, 2], host=True,
                                                                        erased=[[False, False, True]])
    assert values == [[5, 5, 5]] and out == [5] and nerr.tolist() == [0] and not col_err.any() and not mask.any()


SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_evaluate_mirror.cpp")
EXE = os.path.join(ROOT, "build", "shamir_wide_evaluate_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_names_and_cpp_mirror():
    assert "shamir_evaluate_wide_corrected" in P.__all__ and callable(P.shamir_evaluate_wide_corrected)
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in CORRECTED + ERASURES:
            assert name in _ffi._SIGNATURES and hasattr(lib, name), name
            assert f"PVW_API int32_t {name}(" in header
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_EVALUATE_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr


def test_kernel_evaluation_against_horner_under_sanitizers():
    """tests/cpp/shamir_wide_evaluate.cpp: y o M, scale and the coinciding column, the Cauchy entries with their shared inversions
    (a zero difference at each position of a batch), the derivative powers, the three products and the finish rule in the
    kernels' update order and Montgomery forms, sequentially, over pvw_wide.h's own product, accumulator and reduction, against
    Horner on the Berlekamp-Welch polynomial of the sub-row, for every (eps, nu) up to just beyond the bound at t 0..3 x r 0..7,
    targets on and off the points, and one row with r = 200, for each of the 13 primes.  The only sanitizer run: nothing loaded
    into Python is sanitized."""
    exe = os.path.join(ROOT, "build", "shamir_wide_evaluate")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide_evaluate.cpp"), "-o", exe])
    assert len(PRIMES) == 13
    out = subprocess.run([exe] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_EVALUATE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

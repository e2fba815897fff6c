"""Many weighted sums of the same dealers' ciphertexts on the host side: the symbols exist in both builds and the
header, pvw_shamir_lagrange_weights_at equals a restatement in Python integers (and reconstructs packed sharings slot by slot),
pvw_ct_lincomb_many_host equals Python integers and pvw_ct_lincomb_host row by row, a packed handover in miniature decrypts on
the model, argument errors come before the device, and the mirrors check and compile.  No device compute here; the kernels are
checked in tests/test_gpu_ct_lincomb_many.py."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from test_ct_sum_host import GEOMETRIES, _cts, _model_encrypt, _model_setup, _params, _ptr, _rns, _words
from test_ct_lincomb_host import I64_MAX, I64_MIN, _extremes, _host_lincomb, _restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS, INSUFFICIENT_DATA, INVALID_FORMAT, INTERNAL = 1, 17, 18, 19
PLAIN = (1 << 61) - 1
NEW = ["pvw_shamir_lagrange_weights_at", "pvw_ct_lincomb_many_host", "pvw_ct_lincomb_many_device", "pvw_ct_lincomb_many",
       "pvw_decrypt_all_lincomb_many_plain_device", "pvw_decrypt_all_lincomb_many_plain"]
COMBOS = [1, 2, 3, 4, 5, 7, 8, 9, 17]
DEALERS = [1, 8, 63, 64, 65, 130]


def test_both_libraries_and_the_header_have_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name
    for name in ("combine_ciphertexts_many", "decrypt_all_party_combinations_many", "shamir_lagrange_weights_at",
                 "shamir_packed_handover_weights"):
        assert name in P.__all__ and callable(getattr(P, name))


def test_the_row_tile_selector_exists_in_the_tuning_build_only():
    s = subprocess.run(["strings", "-a", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "PVW_SUM_RT" not in s
    assert "PVW_SUM_RT" in subprocess.run(["strings", "-a", _ffi.LIB_TUNING_PATH], capture_output=True, text=True, check=True).stdout


# ---- pvw_shamir_lagrange_weights_at -------------------------------------------------------------------------------------------
def _weights_at(p, indices, targets, fill=77):
    idx, tg = np.array(indices, dtype=np.uint64), np.array(targets, dtype=np.uint64)
    out = np.full((max(len(targets), 1), max(len(indices), 1)), fill, dtype=np.int64)
    rc = _ffi.lib().pvw_shamir_lagrange_weights_at(p, _ptr(idx), len(indices), _ptr(tg), len(targets), _ptr(out))
    return rc, [[int(x) for x in row] for row in out]


def _lagrange_at(points, z, p):
    """the weights at z of `points`, residues in [0, p), by the defining product"""
    out = []
    for xi in points:
        num = den = 1
        for xj in points:
            if xj != xi:
                num, den = num * (z - xj) % p, den * (xi - xj) % p
        out.append(num * pow(den, p - 2, p) % p)
    return out


def _centred(w, p):
    return [x - p if x > p // 2 else x for x in w]


@pytest.mark.parametrize("p", [97, (1 << 31) - 1, PLAIN])
def test_weights_at_any_point_against_python_integers(p):
    rng = random.Random(p)
    for count in (1, 2, 3, 6, 11):
        indices = rng.sample(range(min(p - 1, 60)), count)
        points = [i + 1 for i in indices]
        targets = [p - 1, p - 2, p - 3, indices[0], indices[-1], rng.randrange(p), p - 1, 70 % p]     # 0, -1, -2, two indices, duplicates
        rc, w = _weights_at(p, indices, targets)
        assert rc == 0, _ffi.last_error()
        assert P.shamir_lagrange_weights_at(indices, targets, p) == w
        assert w[0] == P.shamir_lagrange_weights(indices, p) == w[6]
        G = [rng.randrange(p) for _ in range(count)]                    # a random polynomial of degree < count
        ev = lambda x: sum(c * pow(x, e, p) for e, c in enumerate(G)) % p
        for j, t in enumerate(targets):
            z = (t + 1) % p
            assert w[j] == _centred(_lagrange_at(points, z, p), p), (count, j)
            assert all(-p < 2 * x <= p for x in w[j])                    # in (-p/2, p/2]
            assert sum(x * ev(xi) for x, xi in zip(w[j], points)) % p == ev(z)
        for j in (3, 4):                                                 # a target that is an index: that unit vector
            assert w[j] == [1 if i == targets[j] else 0 for i in indices]
        assert P.shamir_packed_handover_weights(indices, p, 3) == w[:3]


@pytest.mark.parametrize("p", [97, (1 << 31) - 1, PLAIN])
def test_packed_weights_applied_to_packed_shares_give_each_secret(p):
    n, K, t = 9, 3, 2
    ctx = _params(n, 2, 8)
    rng = random.Random(p + 1)
    secrets = [[rng.randrange(p) for _ in range(K)] for _ in range(4)]
    seeds = [bytes([d + 7]) * 32 for d in range(4)]
    shares = P.shamir_shares_packed(ctx, secrets, t, p, seeds, host=True)
    holders = [0, 2, 3, 5, 8]                                            # t + K of the n parties
    rows = P.shamir_packed_handover_weights(holders, p, K)
    for d in range(4):
        for m in range(K):
            assert sum(w * int(shares[d][i]) for w, i in zip(rows[m], holders)) % p == secrets[d][m]


def test_weights_at_refusals():
    cases = [((91, [1, 2], [0]), "prime"), ((1, [0], [0]), "prime"), (((1 << 62) + 135, [1, 2], [0]), "2^62"),
             ((PLAIN, [3, 3], [0]), "duplicate party index"), ((97, [96], [0]), "party index out of range"),
             ((97, [1, 2], [5, 97]), "target index out of range"), ((PLAIN, [], [0]), "no shares to reconstruct from"),
             ((PLAIN, [1, 2], []), "no target points")]
    for (p, indices, targets), msg in cases:
        rc, w = _weights_at(p, indices, targets)
        assert rc == INVALID_PARAMETERS and msg in _ffi.last_error(), (p, indices, targets, _ffi.last_error())
        assert all(x == 77 for row in w for x in row)
    lib = _ffi.lib()
    idx, out = np.zeros(1, np.uint64), np.zeros(1, np.int64)
    for args in ((None, 1, _ptr(idx), 1, _ptr(out)), (_ptr(idx), 1, None, 1, _ptr(out)), (_ptr(idx), 1, _ptr(idx), 1, None)):
        assert lib.pvw_shamir_lagrange_weights_at(PLAIN, *args) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
    assert _weights_at(97, [1], [96])[0] == 0                            # p - 1 is a target (the point 0), never an index


# ---- pvw_ct_lincomb_many_host ---------------------------------------------------------------------------------------------------
def _host_many(p, c1s, c2s, rows, valid, lo, hi, name="pvw_ct_lincomb_many_host", lib=None):
    R = len(rows)
    c1 = np.full((R, p.k, p.L, p.l), 5, np.uint64)
    c2 = np.full((R, hi - lo, p.L, p.l), 5, np.uint64)
    cnt = np.full(R, 77, np.uint32)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    w = np.ascontiguousarray(rows, dtype=np.int64)
    rc = getattr(lib or _ffi.lib(), name)(p._h, _ptr(c1s), _ptr(c2s), len(c1s), _ptr(v), _ptr(w), R, lo, hi, _ptr(c1), _ptr(c2), _ptr(cnt))
    return rc, c1, c2, cnt


def weight_rows(rng, moduli, R, D, kind):
    """int64 [R][D]: all ones; uniform over int64; the extremes 0 / +-1 / INT64_MIN / INT64_MAX / +-q_i ... in turn; and in every
    kind with R >= 3 one all-zero row, and one dealer whose weight is zero in some rows only"""
    if kind == "ones":
        w = np.ones((R, D), np.int64)
    elif kind == "uniform":
        w = rng.integers(I64_MIN, I64_MAX, (R, D), dtype=np.int64, endpoint=True)
    else:
        ext = _extremes(moduli)
        w = np.array([[ext[(r * 5 + d) % len(ext)] for d in range(D)] for r in range(R)], dtype=np.int64)
    if R >= 2:
        w[::2, D // 2] = 0                                               # zero in the even rows only
    if R >= 3:
        w[R // 2, :] = 0                                                 # nobody takes part in this row
    return w


@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
@pytest.mark.parametrize("D", DEALERS)
def test_ct_lincomb_many_host_equals_python_integers_and_the_single_call_row_by_row(geom, D):
    n, k, l, moduli = GEOMETRIES[geom]
    p = _params(n, k, l, moduli)
    rng = np.random.default_rng(77 * geom + D)
    ranges = [(0, n), (1, n), (n - 1, n), (0, 1)]
    masks = [None, np.arange(D) % 2 == 0, np.arange(D) == D // 2]
    qs = np.array(moduli, np.uint64).reshape(1, 1, -1, 1)
    words = {kind: (_words(rng, p, D, k, kind), _words(rng, p, D, n, kind)) for kind in ("reduced", "any", "extreme")}
    for step, R in enumerate(COMBOS):
        kind = ("reduced", "any", "extreme")[(step + D) % 3]
        valid = masks[(step + geom) % 3]
        wkind = ("ones", "uniform", "extreme")[step % 3]
        lo, hi = ranges[(step + D) % 4]
        c1s, c2s = (a.copy() for a in words[kind])
        if valid is not None:                                            # a dealer that is masked out is never read: its words do not matter
            c1s[~valid], c2s[~valid] = np.uint64((1 << 64) - 1), np.uint64((1 << 64) - 1)
        rows = weight_rows(rng, moduli, R, D, wkind)
        what = (R, kind, wkind, lo, hi)
        on = [int(np.count_nonzero((rows[r] != 0) & (True if valid is None else valid))) for r in range(R)]
        rc, c1, c2, cnt = _host_many(p, c1s, c2s, rows, valid, lo, hi)
        if not any(on):
            assert rc == INSUFFICIENT_DATA and "No participating dealer" in _ffi.last_error(), what
            assert (c1 == 5).all() and (cnt == 77).all(), what
            continue
        assert rc == 0, _ffi.last_error()
        assert cnt.tolist() == on, what
        assert (c1 < qs).all() and (c2 < qs).all(), what
        for r in range(R):
            if on[r] == 0:
                assert not c1[r].any() and not c2[r].any(), (what, r)
                assert _host_lincomb(p, c1s, c2s, rows[r], valid, lo, hi)[0] == INSUFFICIENT_DATA
                continue
            rc1, s1, s2, scnt = _host_lincomb(p, c1s, c2s, rows[r], valid, lo, hi)
            assert rc1 == 0 and np.array_equal(c1[r], s1) and np.array_equal(c2[r], s2) and scnt == cnt[r], (what, r)
            if R <= 5 or r in (0, R - 1, R // 3):
                w1, w2, _ = _restated(p, c1s, c2s, rows[r], valid, lo, hi)
                assert np.array_equal(c1[r], w1) and np.array_equal(c2[r], w2), (what, r)


# ---- the packed handover in miniature, on the model -----------------------------------------------------------------------------
def test_a_packed_handover_of_model_ciphertexts_decrypts_to_the_new_shares_of_every_slot():
    moduli = M.bench_moduli(17)
    mp, rnd, A, B, sk = _model_setup(moduli, seed=11)                    # n = 3, k = 4, l = 8
    p = _params(mp.n, mp.k, mp.l, moduli)
    K, D, bad = 2, 5, 3
    # the old sharing F of degree 1 holds s_m = F(-m); holder d has y_d = F(d + 1) and re-deals it with a fresh f_d of degree 1
    F = [rnd.randrange(PLAIN), rnd.randrange(PLAIN)]
    y = [(F[0] + F[1] * (d + 1)) % PLAIN for d in range(D)]
    f = [[y[d], rnd.randrange(PLAIN)] for d in range(D)]
    shares = [[(f[d][0] + f[d][1] * (j + 1)) % PLAIN for j in range(mp.n)] for d in range(D)]
    cts = [_model_encrypt(mp, rnd, A, B, s) for s in shares]
    c1s = np.stack([_rns(c1, moduli) for c1, _ in cts])
    c2s = np.stack([_rns(c2, moduli) for _, c2 in cts])
    valid = np.array([d != bad for d in range(D)])
    c1s[bad], c2s[bad] = np.uint64((1 << 64) - 1), np.uint64((1 << 64) - 1)
    holders = [d for d in range(D) if valid[d]]
    lam = P.shamir_packed_handover_weights(holders, PLAIN, K)
    rows = np.zeros((K, D), np.int64)
    rows[:, holders] = lam
    for m in range(K):                                                  # the reference alone stays inside the proven radius
        assert p.lincomb_fits(rows[m], valid) is True
    rc, c1, c2, cnt = _host_many(p, c1s, c2s, rows, valid, 0, mp.n)
    assert rc == 0 and cnt.tolist() == [len(holders)] * K, _ffi.last_error()
    for m in range(K):
        comb_c1 = [M.from_rns(c1[m][j].tolist(), moduli) for j in range(mp.k)]
        new = []
        for j in range(mp.n):
            noisy = M.decrypt_noisy(mp, comb_c1, M.from_rns(c2[m][j].tolist(), moduli), sk[j])
            r = P.decode_scalar_pvw_plain_host(p, _rns([noisy], moduli), plain_modulus=PLAIN)
            assert int(r.values[0]) == sum(int(rows[m][d]) * shares[d][j] for d in holders) % PLAIN, (m, j)
            new.append(int(r.values[0]))
        # the new shares are a degree-1 sharing of s_m = F(-m): any two of them give it back
        assert P.shamir_reconstruct([0, 2], [[new[0], new[2]]], PLAIN)[0] == (F[0] - m * F[1]) % PLAIN


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def _many_call(lib, name, p, c1s, c2s, D, valid, w, R, lo, hi, c1, c2, cnt=None):
    args = [p._h, c1s, c2s, D, valid, w, R, lo, hi, c1, c2, cnt] + ([None] if name.endswith("_device") else [])
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", ["pvw_ct_lincomb_many", "pvw_ct_lincomb_many_device", "pvw_ct_lincomb_many_host"])
def test_ct_lincomb_many_argument_errors_come_before_the_device(name):
    lib = _ffi.lib()
    p = _params()
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    c1, c2 = np.zeros((2, p.k, p.L, p.l), np.uint64), np.zeros((2, p.n, p.L, p.l), np.uint64)
    a, b, x, y, w = _ptr(c1s), _ptr(c2s), _ptr(c1), _ptr(c2), _ptr(np.ones((2, 3), np.int64))
    cases = [
        ((None, b, 3, w, 2, 0, 6, x, y), "NULL argument"), ((a, None, 3, w, 2, 0, 6, x, y), "NULL argument"),
        ((a, b, 3, w, 2, 0, 6, None, y), "NULL argument"), ((a, b, 3, w, 2, 0, 6, x, None), "NULL argument"),
        ((a, b, 3, None, 2, 0, 6, x, y), "NULL argument"),
        ((a, b, 0, w, 2, 0, 6, x, y), "No ciphertexts provided"), ((a, b, 1 << 32, w, 2, 0, 6, x, y), "fewer than 2^32 dealers"),
        ((a, b, 3, w, 2, 2, 2, x, y), "empty row range"), ((a, b, 3, w, 2, 4, 3, x, y), "row_lo > row_hi"),
        ((a, b, 3, w, 2, 5, 7, x, y), "Row index 6 exceeds maximum 5"),
        ((a, b, 3, w, 0, 0, 6, x, y), "num_combos must be at least 1"),
    ]
    if name.endswith("_device"):
        cases.append(((a, b, 3, w, 1 << 31, 0, 6, x, y), "num_combos must be below 2^31"))
    for (q1, q2, D, ww, R, lo, hi, o1, o2), msg in cases:
        assert _many_call(lib, name, p, q1, q2, D, None, ww, R, lo, hi, o1, o2) == INVALID_PARAMETERS, msg
        assert msg in _ffi.last_error()
    if name != "pvw_ct_lincomb_many_device":     # the host knows mask and weights: nobody in ANY row is refused before any device work
        cnt = np.full(2, 77, np.uint32)
        zero = _ptr(np.zeros((2, 3), np.int64))
        assert _many_call(lib, name, p, a, b, 3, _ptr(np.zeros(3, np.uint8)), w, 2, 0, 6, x, y, _ptr(cnt)) == INSUFFICIENT_DATA
        assert _many_call(lib, name, p, a, b, 3, None, zero, 2, 0, 6, x, y, _ptr(cnt)) == INSUFFICIENT_DATA
        split = _ptr(np.array([[0, 4, -4], [0, 0, 9]], np.int64))
        assert _many_call(lib, name, p, a, b, 3, _ptr(np.array([1, 0, 0], np.uint8)), split, 2, 0, 6, x, y, _ptr(cnt)) == INSUFFICIENT_DATA
        assert "No participating dealer" in _ffi.last_error() and (cnt == 77).all()
    assert not c1.any() and not c2.any()


def test_decrypt_all_lincomb_many_argument_errors_come_before_the_device():
    lib = _ffi.lib()
    p = _params()
    sk = np.zeros((2, p.k, p.l), np.int64)
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    out = np.zeros((2, 2), np.uint64)
    s, a, b, o, none, w = _ptr(sk), _ptr(c1s), _ptr(c2s), _ptr(out), _ptr(np.zeros(3, np.uint8)), _ptr(np.ones((2, 3), np.int64))
    zero = _ptr(np.zeros((2, 3), np.int64))
    for R in (1, 2):                                                    # R = 1 is the mirrored call: the same refusals
        for fn, tail in (("pvw_decrypt_all_lincomb_many_plain", []), ("pvw_decrypt_all_lincomb_many_plain_device", [None])):
            al = lambda lo, hi, sk_, c1_, c2_, D, v, w_, rep, o_, plain=(0, 0, None): getattr(lib, fn)(
                p._h, lo, hi, sk_, c1_, c2_, D, v, w_, R, rep, o_, None, None, None, *plain, *tail)
            assert al(1, 3, None, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and al(1, 3, s, a, b, 0, None, w, 1, o) == INVALID_PARAMETERS
            assert al(1, 3, s, a, b, 3, None, None, 1, o) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
            assert al(3, 3, s, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and "empty party range" in _ffi.last_error()
            assert al(5, 7, s, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and "Party index 6 exceeds maximum 5" in _ffi.last_error()
            assert al(1, 3, s, a, b, 1 << 32, None, w, 1, o) == INVALID_PARAMETERS and al(1, 3, s, a, b, 3, None, w, 7, o) == INVALID_FORMAT
            assert al(1, 3, s, a, b, 3, None, w, 1, o, plain=(1, 0, None)) == INVALID_PARAMETERS
            assert al(1, 3, s, a, b, 3, None, w, 1, o, plain=(0, 1, None)) == INVALID_PARAMETERS
        many = lambda v, w_: lib.pvw_decrypt_all_lincomb_many_plain(p._h, 1, 3, s, a, b, 3, v, w_, R, 1, o, None, None, None, 0, 0, None)
        assert many(none, w) == INSUFFICIENT_DATA and many(None, zero) == INSUFFICIENT_DATA
    for fn, tail in (("pvw_decrypt_all_lincomb_many_plain", []), ("pvw_decrypt_all_lincomb_many_plain_device", [None])):
        assert getattr(lib, fn)(p._h, 1, 3, s, a, b, 3, None, w, 0, 1, o, None, None, None, 0, 0, None, *tail) == INVALID_PARAMETERS
        assert "num_combos must be at least 1" in _ffi.last_error()
    assert lib.pvw_decrypt_all_lincomb_many_plain_device(p._h, 1, 3, s, a, b, 3, None, w, 1 << 31, 1, o, None, None, None, 0, 0, None,
                                                         None) == INVALID_PARAMETERS
    assert "num_combos must be below 2^31" in _ffi.last_error()
    assert not out.any()


@pytest.mark.skipif(P.device_available(), reason="a device is present: the calls run (tests/test_gpu_ct_lincomb_many.py)")
def test_valid_arguments_without_a_device_fail_loudly():
    lib = _ffi.lib()
    p = _params()
    sk = np.zeros((2, p.k, p.l), np.int64)
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    c1, c2, out = np.zeros((2, p.k, p.L, p.l), np.uint64), np.zeros((2, p.n, p.L, p.l), np.uint64), np.zeros((2, 2), np.uint64)
    s, a, b, x, y, o, w = _ptr(sk), _ptr(c1s), _ptr(c2s), _ptr(c1), _ptr(c2), _ptr(out), _ptr(np.ones((2, 3), np.int64))
    calls = [
        lambda: lib.pvw_ct_lincomb_many(p._h, a, b, 3, None, w, 2, 0, 6, x, y, None),
        lambda: lib.pvw_ct_lincomb_many_device(p._h, a, b, 3, None, w, 2, 0, 6, x, y, None, None),
        lambda: lib.pvw_decrypt_all_lincomb_many_plain(p._h, 1, 3, s, a, b, 3, None, w, 2, 1, o, None, None, None, PLAIN, 0, None),
        lambda: lib.pvw_decrypt_all_lincomb_many_plain_device(p._h, 1, 3, s, a, b, 3, None, w, 2, 1, o, None, None, None, PLAIN, 0, None, None),
    ]
    for call in calls:
        assert call() == INTERNAL and "no CPU fallback" in _ffi.last_error()


# ---- mirrors ------------------------------------------------------------------------------------------------------------------
def test_python_mirror_checks_before_the_device_and_runs_the_host_form():
    p = _params()
    key = P.SecretKey(p, np.zeros((p.k, p.l), np.int64))
    parties = [P.Party(i, key) for i in range(p.n)]
    for fn in (lambda c, w, **kw: P.combine_ciphertexts_many(c, w, **kw),
               lambda c, w, **kw: P.decrypt_all_party_combinations_many(c, w, parties, **kw)):
        with pytest.raises(P.PvwError, match="No ciphertexts provided"):
            fn([], [[]])
        with pytest.raises(P.PvwError, match="num_combos must be at least 1"):
            fn(_cts(p, 3), [])
        with pytest.raises(P.PvwError, match=r"DimensionMismatch: weight_rows\[1\]: expected 3 weights, got 2"):
            fn(_cts(p, 3), [[1, 1, 1], [1, 1]])
        with pytest.raises(P.PvwError, match="outside the int64 range"):
            fn(_cts(p, 3), [[1, 1, 1], [1, 1 << 63, 1]])
        with pytest.raises(P.PvwError, match="InsufficientData: No valid dealer"):
            fn(_cts(p, 3), [[1, 1, 1]], valid=[0, 0, 0])
        with pytest.raises(P.PvwError, match="InsufficientData: No participating dealer"):
            fn(_cts(p, 3), [[0, 5, 0], [0, 0, 0]], valid=[1, 0, 1])
    with pytest.raises(P.PvwError, match="consecutive"):
        P.decrypt_all_party_combinations_many(_cts(p, 2), [[1, 1]], [parties[0], parties[2]])
    assert P.decrypt_all_party_combinations_many(_cts(p, 2), [[1, 1], [2, 0]], []).values.shape == (0, 2)
    rng = np.random.default_rng(3)
    cts = [P.PvwCiphertext(rng.integers(0, 1 << 64, (p.k, p.L, p.l), dtype=np.uint64),
                           rng.integers(0, 1 << 64, (p.n, p.L, p.l), dtype=np.uint64), p, P.REPR_POWER) for _ in range(4)]
    rows = [[I64_MIN, 3, -7, I64_MAX], [0, 0, 5, 0], [1, 0, 0, -1]]
    combs = P.combine_ciphertexts_many(cts, rows, valid=[1, 1, 0, 1], host=True)
    assert len(combs) == 3 and not combs[1].c1.any() and not combs[1].c2.any()      # row 1: its only dealer is masked out
    for r in (0, 2):
        one = P.combine_ciphertexts(cts, rows[r], valid=[1, 1, 0, 1], host=True)
        assert combs[r].params is p and combs[r].repr == P.REPR_POWER
        assert np.array_equal(combs[r].c1, one.c1) and np.array_equal(combs[r].c2, one.c2)


def test_cpp_mirror_compiles_against_the_header():
    exe = os.path.join(ROOT, "build", "ct_lincomb_many_cpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "ct_lincomb_many.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "pvw_rs_amd"), "-lpvw_hip", "-Wl,-rpath," + os.path.join(ROOT, "pvw_rs_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)

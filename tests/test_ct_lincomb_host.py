"""Weighted sums of dealers' ciphertexts on the host side: the symbols exist in both builds, pvw_ct_lincomb_host
equals a restatement in Python integers over every kind of weight, the combination of model ciphertexts with Lagrange weights
decodes to sum w_d m_d mod p inside the radius pvw_ctx_lincomb_fits describes, pvw_shamir_lagrange_weights are the centred
weights pvw_shamir_reconstruct uses, argument errors come before the device, and the mirrors check and compile.  No device
compute here; the kernels are checked in tests/test_gpu_ct_lincomb.py."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import EXAMPLE_MODULI
from test_ct_sum_host import GEOMETRIES, _cts, _host_sum, _model_encrypt, _model_setup, _params, _ptr, _rns, _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS, INSUFFICIENT_DATA, INVALID_FORMAT, INTERNAL = 1, 17, 18, 19
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
PLAIN = (1 << 61) - 1
NEW = ["pvw_ct_lincomb_device", "pvw_ct_lincomb", "pvw_ct_lincomb_host", "pvw_decrypt_lincomb_plain", "pvw_decrypt_lincomb_plain_device",
       "pvw_decrypt_lincomb_device_sk_plain", "pvw_decrypt_all_lincomb_plain", "pvw_decrypt_all_lincomb_plain_device",
       "pvw_ctx_lincomb_fits", "pvw_shamir_lagrange_weights"]


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name


def test_the_shipped_library_has_no_new_switch():
    # the slice count is ct_sum_slices' (PVW_SUM_SPLIT, tuning build only): the combination adds no environment lookup
    s = subprocess.run(["strings", "-a", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "PVW_SUM_SPLIT" not in s and "PVW_LINCOMB" not in s
    assert "PVW_LINCOMB" not in subprocess.run(["strings", "-a", _ffi.LIB_TUNING_PATH], capture_output=True, text=True, check=True).stdout


# ---- pvw_ct_lincomb_host against Python integers ----------------------------------------------------------------------
def _restated(p, c1s, c2s, weights, valid, lo, hi):
    """out = sum over the participating dealers of w_d * in_d, word by word mod q of the word's limb, in Python integers"""
    q = np.array([int(x) for x in p.moduli()], dtype=object).reshape(1, -1, 1)
    on = [d for d in range(len(c1s)) if (valid is None or valid[d]) and int(weights[d]) != 0]
    c1 = sum((int(weights[d]) * c1s[d].astype(object) for d in on), np.zeros(c1s.shape[1:], dtype=object)) % q
    c2 = sum((int(weights[d]) * c2s[d, lo:hi].astype(object) for d in on), np.zeros(c2s[0, lo:hi].shape, dtype=object)) % q
    return c1.astype(np.uint64), c2.astype(np.uint64), len(on)


def _host_lincomb(p, c1s, c2s, weights, valid, lo, hi):
    c1 = np.zeros((p.k, p.L, p.l), np.uint64)
    c2 = np.zeros((hi - lo, p.L, p.l), np.uint64)
    cnt = C.c_uint32(77)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    w = np.ascontiguousarray(weights, dtype=np.int64)
    rc = _ffi.lib().pvw_ct_lincomb_host(p._h, _ptr(c1s), _ptr(c2s), len(c1s), _ptr(v), _ptr(w), lo, hi, _ptr(c1), _ptr(c2), C.byref(cnt))
    return rc, c1, c2, cnt.value


def _extremes(moduli):
    """0, +-1, the ends of int64, and for every limb +-q, +-(q - 1) and a multiple of q"""
    ext = [0, 1, -1, I64_MIN, I64_MAX]
    for q in (int(x) for x in moduli):
        big = (I64_MAX // q) * q                                   # the largest multiple of q in int64
        ext += [q, -q, q - 1, -(q - 1), big, -big]
    return ext


def _weight_sets(rng, moduli, D):
    """(name, int64 [D]): all 1; uniform over int64; the extremes, rotated so that every one reaches every position in turn;
    a set with zeros"""
    ext = _extremes(moduli)
    sets = [("ones", np.ones(D, np.int64)), ("uniform", rng.integers(I64_MIN, I64_MAX, D, dtype=np.int64, endpoint=True))]
    for shift in range(len(ext) if D < len(ext) else 1):
        sets.append((f"extreme{shift}", np.array([ext[(d + shift) % len(ext)] for d in range(D)], dtype=np.int64)))
    z = rng.integers(-5, 6, D, dtype=np.int64)
    z[::3] = 0
    sets.append(("zeros", z))
    return sets


def _masks(D):
    return [None, np.arange(D) % 2 == 0, np.arange(D) == D // 2]


@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
@pytest.mark.parametrize("D", [1, 2, 7, 130])
def test_ct_lincomb_host_equals_python_integers(geom, D):
    n, k, l, moduli = GEOMETRIES[geom]
    p = _params(n, k, l, moduli)
    rng = np.random.default_rng(1000 * geom + D)
    ranges = [(0, n), (1, n), (n - 1, n), (0, 1)]
    qs = np.array(moduli, np.uint64).reshape(1, -1, 1)
    sets = _weight_sets(rng, moduli, D)
    step = 0
    for i, kind in enumerate(["reduced", "any", "extreme"]):
        c1s, c2s = _words(rng, p, D, k, kind), _words(rng, p, D, n, kind)
        for j, valid in enumerate(_masks(D)):
            for name, w in sets:
                if name.startswith("extreme") and name != "extreme0" and (kind, j) != ("any", 0):
                    continue                                        # the rotations once: any words, every dealer
                step += 1
                lo, hi = ranges[step % len(ranges)]
                rc, c1, c2, cnt = _host_lincomb(p, c1s, c2s, w, valid, lo, hi)
                w1, w2, on = _restated(p, c1s, c2s, w, valid, lo, hi)
                what = (kind, j, name, lo, hi)
                if on == 0:
                    assert rc == INSUFFICIENT_DATA and "No participating dealer" in _ffi.last_error() and cnt == 77, what
                    continue
                assert rc == 0, _ffi.last_error()
                assert np.array_equal(c1, w1) and np.array_equal(c2, w2), what
                assert cnt == on, what
                assert (c1 < qs).all() and (c2 < qs).all(), what
                if name == "ones":
                    rc, s1, s2, scnt = _host_sum(p, c1s, c2s, valid, lo, hi)
                    assert rc == 0 and np.array_equal(c1, s1) and np.array_equal(c2, s2) and scnt == cnt, what


def test_extreme_words_and_weights_everywhere_exercise_the_wraps():
    # 130 dealers of 2^64 - 1 in every position times INT64_MIN: every partial sum of the lazy accumulator wraps
    p = _params(3, 2, 8, M.bench_moduli(2))
    c1s = np.full((130, p.k, p.L, p.l), (1 << 64) - 1, np.uint64)
    c2s = np.full((130, p.n, p.L, p.l), (1 << 64) - 1, np.uint64)
    rc, c1, c2, cnt = _host_lincomb(p, c1s, c2s, np.full(130, I64_MIN, np.int64), None, 0, p.n)
    assert rc == 0 and cnt == 130
    for i, q in enumerate(int(x) for x in p.moduli()):
        want = np.uint64(130 * ((1 << 64) - 1) * I64_MIN % q)
        assert (c1[:, i] == want).all() and (c2[:, i] == want).all()


# ---- homomorphism on the model ----------------------------------------------------------------------------------------
def _lagrange_at_zero(points, p):
    out = []
    for xi in points:
        num = den = 1
        for xj in points:
            if xj != xi:
                num, den = num * xj % p, den * (xj - xi) % p
        out.append(num * pow(den, p - 2, p) % p)
    return out


def _centred(w, p):
    return [x - p if x > p // 2 else x for x in w]


def _model_combination(moduli, D, weights, seed=5):
    """D model ciphertexts of field-sized shares, combined by pvw_ct_lincomb_host: (p, mp, shares, sk, cts, c1, c2)"""
    mp, rnd, A, B, sk = _model_setup(moduli, seed=seed)
    p = _params(mp.n, mp.k, mp.l, moduli)
    shares = [[rnd.randrange(PLAIN) for _ in range(mp.n)] for _ in range(D)]
    cts = [_model_encrypt(mp, rnd, A, B, s) for s in shares]
    c1s = np.stack([_rns(c1, moduli) for c1, _ in cts])
    c2s = np.stack([_rns(c2, moduli) for _, c2 in cts])
    rc, c1, c2, cnt = _host_lincomb(p, c1s, c2s, weights, None, 0, mp.n)
    assert rc == 0 and cnt == sum(1 for w in weights if w), _ffi.last_error()
    return p, mp, shares, sk, cts, c1, c2


def _ring_scale(poly, w, Q):
    return [c * w % Q for c in poly]


def _check_combination(moduli, D, weights):
    p, mp, shares, sk, cts, c1, c2 = _model_combination(moduli, D, weights)
    # the ring arithmetic of the model, polynomial by polynomial
    for j in range(mp.k):
        acc = [0] * mp.l
        for d in range(D):
            acc = M.ring_add(acc, _ring_scale(cts[d][0][j], weights[d], mp.Q), mp.Q)
        assert np.array_equal(c1[j], np.array(M.to_rns(acc, moduli), np.uint64))
    for i in range(mp.n):
        acc = [0] * mp.l
        for d in range(D):
            acc = M.ring_add(acc, _ring_scale(cts[d][1][i], weights[d], mp.Q), mp.Q)
        assert np.array_equal(c2[i], np.array(M.to_rns(acc, moduli), np.uint64))
    comb_c1 = [M.from_rns(c1[j].tolist(), moduli) for j in range(mp.k)]
    for i in range(mp.n):
        noisy = M.decrypt_noisy(mp, comb_c1, M.from_rns(c2[i].tolist(), moduli), sk[i])
        r = P.decode_scalar_pvw_plain_host(p, _rns([noisy], moduli), plain_modulus=PLAIN)
        assert int(r.values[0]) == sum(w * shares[d][i] for d, w in enumerate(weights)) % PLAIN, i
    return p


@pytest.mark.parametrize("D", [1, 5, 64])
@pytest.mark.parametrize("centred", [True, False])
def test_the_combination_of_model_ciphertexts_decodes_to_the_combination_of_the_plaintexts(D, centred):
    lam = _lagrange_at_zero(list(range(1, D + 1)), PLAIN)
    weights = _centred(lam, PLAIN) if centred else lam
    assert sum(weights) % PLAIN == 1
    p = _check_combination(M.bench_moduli(17), D, weights)
    assert p.lincomb_fits(weights) is True
    # The same weights at five limbs (R = 2^38): field-sized ones leave the radius.  The weights at 0 of the points 1..D are the
    # integers (-1)^(i-1) C(D, i), so the CENTRED ones stay small while C(D, i) < p / 2: at D = 5 they are 5, -10, 10, -5, 1 and
    # fit (and decode); at D = 64 they are field-sized, as every residue in [0, p) of a negative weight is.
    m5 = M.bench_moduli(5)
    small = _params(3, 4, 8, m5)
    mp5 = M.Params(3, 4, 8, m5, 0.5, 100, 200)
    R5 = (mp5.Q - 1) // (2 * (mp5.delta_power_l_minus_1 + 1))
    inside = sum(abs(w) for w in weights) * small.noise_bound() <= R5
    assert small.lincomb_fits(weights) is inside
    assert inside is (D == 1 or (centred and D == 5))
    if inside:
        _check_combination(m5, D, weights)
    tiny = [(-1) ** d * (1 + d % 3) for d in range(D)]
    assert _check_combination(M.bench_moduli(5), D, tiny).lincomb_fits(tiny) is True


# ---- pvw_ctx_lincomb_fits ---------------------------------------------------------------------------------------------------
def _fits(p, weights, valid=None, n=None):
    w = np.ascontiguousarray(weights, dtype=np.int64)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    out = C.c_uint32(7)
    rc = _ffi.lib().pvw_ctx_lincomb_fits(p._h, _ptr(w), len(w) if n is None else n, _ptr(v), C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("moduli", [M.bench_moduli(5), M.bench_moduli(9), EXAMPLE_MODULI])
def test_lincomb_fits_is_the_radius_over_the_noise_bound_at_the_boundary(moduli):
    p = _params(3, 4, 8, moduli)
    mp = M.Params(3, 4, 8, moduli, 0.5, 100, 200)
    R = (mp.Q - 1) // (2 * (mp.delta_power_l_minus_1 + 1))
    nb = p.noise_bound()
    most = R // nb                                                   # the largest sum of |w| that fits: most * nb <= R < (most + 1) * nb
    assert nb > 0 and 10 < most < I64_MAX
    at = [most - 6, -1, 2, -3]                                       # one big weight plus small ones, exactly at the boundary
    assert sum(abs(x) for x in at) * nb <= R < (sum(abs(x) for x in at) + 1) * nb
    assert _fits(p, at) == (0, 1)
    assert _fits(p, at + [1]) == (0, 0) and _fits(p, at + [-1]) == (0, 0)
    assert _fits(p, [-most]) == (0, 1) and _fits(p, [-most - 1]) == (0, 0)
    # a dealer that is masked out or has weight 0 does not count
    assert _fits(p, at + [5, 0], [1] * len(at) + [0, 1]) == (0, 1)
    assert _fits(p, at + [5, 0], [1] * len(at) + [1, 1]) == (0, 0)
    assert _fits(p, [0, 0]) == (0, 1)
    assert p.lincomb_fits(at) is True and p.lincomb_fits(at + [1]) is False
    lib = _ffi.lib()
    out = C.c_uint32()
    w = np.array([1], np.int64)
    assert lib.pvw_ctx_lincomb_fits(None, _ptr(w), 1, None, C.byref(out)) == INVALID_PARAMETERS
    assert lib.pvw_ctx_lincomb_fits(p._h, None, 1, None, C.byref(out)) == INVALID_PARAMETERS
    assert lib.pvw_ctx_lincomb_fits(p._h, _ptr(w), 1, None, None) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()


def test_lincomb_fits_takes_int64_min_as_two_to_the_63():
    # a geometry whose radius holds a handful of weights of magnitude 2^63
    for limbs in range(9, 18):
        moduli = M.bench_moduli(limbs)
        p = _params(3, 4, 8, moduli)
        mp = M.Params(3, 4, 8, moduli, 0.5, 100, 200)
        R = (mp.Q - 1) // (2 * (mp.delta_power_l_minus_1 + 1))
        cnt = R // (p.noise_bound() << 63)
        if 1 <= cnt < 1 << 12:
            break
    assert 1 <= cnt < 1 << 12, limbs
    assert _fits(p, [I64_MIN] * cnt) == (0, 1) and _fits(p, [I64_MIN] * (cnt + 1)) == (0, 0)
    assert _fits(p, [I64_MIN] * cnt + [I64_MAX]) == (0, 0)


# ---- pvw_shamir_lagrange_weights --------------------------------------------------------------------------------------------
def _lagrange(p, indices):
    idx = np.array(indices, dtype=np.uint64)
    out = np.full(len(indices), 77, dtype=np.int64)
    rc = _ffi.lib().pvw_shamir_lagrange_weights(p, _ptr(idx), len(indices), _ptr(out))
    return rc, [int(x) for x in out]


@pytest.mark.parametrize("p", [PLAIN, 97, 2147483647, 7])
def test_lagrange_weights_are_centred_and_reconstruct(p):
    rng = random.Random(p)
    for count in (1, 2, 3, 5):
        indices = rng.sample(range(min(p - 1, 40)), count)
        rc, w = _lagrange(p, indices)
        assert rc == 0, _ffi.last_error()
        assert w == _centred(_lagrange_at_zero([i + 1 for i in indices], p), p)
        assert all(-(p // 2) <= x <= p // 2 for x in w) and sum(w) % p == 1
        assert P.shamir_lagrange_weights(indices, p) == w
        # they reconstruct what pvw_shamir_shares_host deals
        n = max(indices) + 1
        if n < p and count - 1 < n:
            ctx = _params(n, 2, 8)
            secrets = [rng.randrange(p) for _ in range(3)]
            seeds = [bytes([d + 1]) * 32 for d in range(3)]
            shares = P.shamir_shares(ctx, secrets, count - 1, p, seeds, host=True)
            for d in range(3):
                assert sum(x * int(shares[d][i]) for x, i in zip(w, indices)) % p == secrets[d]


def test_lagrange_weights_argument_errors_are_those_of_reconstruct():
    lib = _ffi.lib()
    cases = [((PLAIN, []), "no shares to reconstruct from"), ((PLAIN, [3, 3]), "duplicate party index"),
             ((97, [96]), "party index out of range"), ((91, [1, 2]), "prime"), ((1, [0]), "prime"),
             (((1 << 62) + 135, [1, 2]), "2^62")]
    for (p, indices), msg in cases:
        rc, w = _lagrange(p, indices)
        assert rc == INVALID_PARAMETERS and msg in _ffi.last_error(), (p, indices, _ffi.last_error())
        assert all(x == 77 for x in w)
        # the same refusal as pvw_shamir_reconstruct's
        idx, sh, out = np.array(indices, np.uint64), np.zeros(max(len(indices), 1), np.uint64), np.zeros(1, np.uint64)
        assert lib.pvw_shamir_reconstruct(p, _ptr(idx), _ptr(sh), len(indices), 1, _ptr(out)) == INVALID_PARAMETERS
        assert msg in _ffi.last_error()
    out = np.zeros(1, np.int64)
    assert lib.pvw_shamir_lagrange_weights(PLAIN, None, 1, _ptr(out)) == INVALID_PARAMETERS
    assert lib.pvw_shamir_lagrange_weights(PLAIN, _ptr(np.zeros(1, np.uint64)), 1, None) == INVALID_PARAMETERS
    assert "NULL argument" in _ffi.last_error()


# ---- argument errors ----------------------------------------------------------------------------------------------------
def _comb_call(lib, name, p, c1s, c2s, D, valid, w, lo, hi, c1, c2):
    args = [p._h, c1s, c2s, D, valid, w, lo, hi, c1, c2, None] + ([None] if name.endswith("_device") else [])
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", ["pvw_ct_lincomb", "pvw_ct_lincomb_device", "pvw_ct_lincomb_host"])
def test_ct_lincomb_argument_errors_come_before_the_device(name):
    lib = _ffi.lib()
    p = _params()
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    c1, c2 = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64)
    a, b, x, y, w = _ptr(c1s), _ptr(c2s), _ptr(c1), _ptr(c2), _ptr(np.ones(3, np.int64))
    cases = [
        ((None, b, 3, w, 0, 6, x, y), "NULL argument"), ((a, None, 3, w, 0, 6, x, y), "NULL argument"),
        ((a, b, 3, w, 0, 6, None, y), "NULL argument"), ((a, b, 3, w, 0, 6, x, None), "NULL argument"),
        ((a, b, 3, None, 0, 6, x, y), "NULL argument"),
        ((a, b, 0, w, 0, 6, x, y), "No ciphertexts provided"), ((a, b, 1 << 32, w, 0, 6, x, y), "fewer than 2^32 dealers"),
        ((a, b, 3, w, 2, 2, x, y), "empty row range"), ((a, b, 3, w, 4, 3, x, y), "row_lo > row_hi"),
        ((a, b, 3, w, 5, 7, x, y), "Row index 6 exceeds maximum 5"),
    ]
    for (q1, q2, D, ww, lo, hi, o1, o2), msg in cases:
        assert _comb_call(lib, name, p, q1, q2, D, None, ww, lo, hi, o1, o2) == INVALID_PARAMETERS, msg
        assert msg in _ffi.last_error()
    if name != "pvw_ct_lincomb_device":     # the host knows mask and weights: no participating dealer is refused before any device work
        assert _comb_call(lib, name, p, a, b, 3, _ptr(np.zeros(3, np.uint8)), w, 0, 6, x, y) == INSUFFICIENT_DATA
        assert _comb_call(lib, name, p, a, b, 3, None, _ptr(np.zeros(3, np.int64)), 0, 6, x, y) == INSUFFICIENT_DATA
        assert _comb_call(lib, name, p, a, b, 3, _ptr(np.array([1, 0, 0], np.uint8)), _ptr(np.array([0, 4, -4], np.int64)), 0, 6, x, y) == INSUFFICIENT_DATA
        assert "No participating dealer" in _ffi.last_error()
    assert not c1.any() and not c2.any()


def test_decrypt_lincomb_argument_errors_come_before_the_device():
    lib = _ffi.lib()
    p = _params()
    sk = np.zeros((2, p.k, p.l), np.int64)
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    out, wide = np.zeros(2, np.uint64), np.zeros(8, np.uint64)
    s, a, b, o, none, w = _ptr(sk), _ptr(c1s), _ptr(c2s), _ptr(out), _ptr(np.zeros(3, np.uint8)), _ptr(np.ones(3, np.int64))
    zero = _ptr(np.zeros(3, np.int64))
    one = lambda *x, plain=(0, 0, None): lib.pvw_decrypt_lincomb_plain(p._h, *x, None, None, None, *plain)
    assert one(None, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and one(s, a, b, 3, None, w, 1, None) == INVALID_PARAMETERS
    assert one(s, a, b, 3, None, None, 1, o) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
    assert one(s, a, b, 0, None, w, 1, o) == INVALID_PARAMETERS and "No ciphertexts provided" in _ffi.last_error()
    assert one(s, a, b, 1 << 32, None, w, 1, o) == INVALID_PARAMETERS and one(s, a, b, 3, None, w, 7, o) == INVALID_FORMAT
    assert one(s, a, b, 3, none, w, 1, o) == INSUFFICIENT_DATA and one(s, a, b, 3, None, zero, 1, o) == INSUFFICIENT_DATA
    assert one(s, a, b, 3, None, w, 1, o, plain=(1, 0, None)) == INVALID_PARAMETERS            # the plain options' own rules
    assert one(s, a, b, 3, None, w, 1, o, plain=(1 << 62, 0, None)) == INVALID_PARAMETERS
    assert one(s, a, b, 3, None, w, 1, o, plain=(0, 1, None)) == INVALID_PARAMETERS
    assert one(s, a, b, 3, None, w, 1, o, plain=(0, 99, _ptr(wide))) == INVALID_PARAMETERS
    dev = lambda fn, key, *x: getattr(lib, fn)(p._h, key, *x, None, None, None, 0, 0, None, None)
    for fn in ("pvw_decrypt_lincomb_plain_device", "pvw_decrypt_lincomb_device_sk_plain"):
        assert dev(fn, None, a, b, 3, None, w, 1, None, o) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
        assert dev(fn, s, a, b, 3, None, None, 1, None, o) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
    assert dev("pvw_decrypt_lincomb_plain_device", s, a, b, 0, None, w, 1, None, o) == INVALID_PARAMETERS
    assert dev("pvw_decrypt_lincomb_plain_device", s, a, b, 3, None, w, 9, None, o) == INVALID_FORMAT
    for fn, tail in (("pvw_decrypt_all_lincomb_plain", []), ("pvw_decrypt_all_lincomb_plain_device", [None])):
        al = lambda lo, hi, *x: getattr(lib, fn)(p._h, lo, hi, *x, None, None, None, 0, 0, None, *tail)
        assert al(1, 3, None, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and al(1, 3, s, a, b, 0, None, w, 1, o) == INVALID_PARAMETERS
        assert al(1, 3, s, a, b, 3, None, None, 1, o) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
        assert al(3, 3, s, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and "empty party range" in _ffi.last_error()
        assert al(5, 7, s, a, b, 3, None, w, 1, o) == INVALID_PARAMETERS and "Party index 6 exceeds maximum 5" in _ffi.last_error()
        assert al(1, 3, s, a, b, 1 << 32, None, w, 1, o) == INVALID_PARAMETERS and al(1, 3, s, a, b, 3, None, w, 7, o) == INVALID_FORMAT
    assert lib.pvw_decrypt_all_lincomb_plain(p._h, 1, 3, s, a, b, 3, none, w, 1, o, None, None, None, 0, 0, None) == INSUFFICIENT_DATA
    assert lib.pvw_decrypt_all_lincomb_plain(p._h, 1, 3, s, a, b, 3, None, zero, 1, o, None, None, None, 0, 0, None) == INSUFFICIENT_DATA
    assert not out.any()


@pytest.mark.skipif(P.device_available(), reason="a device is present: the calls run (tests/test_gpu_ct_lincomb.py)")
def test_valid_arguments_without_a_device_fail_loudly():
    lib = _ffi.lib()
    p = _params()
    sk = np.zeros((2, p.k, p.l), np.int64)
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    c1, c2, out = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64), np.zeros(2, np.uint64)
    s, a, b, x, y, o, w = _ptr(sk), _ptr(c1s), _ptr(c2s), _ptr(c1), _ptr(c2), _ptr(out), _ptr(np.ones(3, np.int64))
    calls = [
        lambda: lib.pvw_ct_lincomb(p._h, a, b, 3, None, w, 0, 6, x, y, None),
        lambda: lib.pvw_ct_lincomb_device(p._h, a, b, 3, None, w, 0, 6, x, y, None, None),
        lambda: lib.pvw_decrypt_lincomb_plain(p._h, s, a, b, 3, None, w, 1, o, None, None, None, PLAIN, 0, None),
        lambda: lib.pvw_decrypt_lincomb_plain_device(p._h, s, a, b, 3, None, w, 1, None, o, None, None, None, PLAIN, 0, None, None),
        lambda: lib.pvw_decrypt_all_lincomb_plain(p._h, 1, 3, s, a, b, 3, None, w, 1, o, None, None, None, PLAIN, 0, None),
        lambda: lib.pvw_decrypt_all_lincomb_plain_device(p._h, 1, 3, s, a, b, 3, None, w, 1, o, None, None, None, PLAIN, 0, None, None),
    ]
    for call in calls:
        assert call() == INTERNAL and "no CPU fallback" in _ffi.last_error()


# ---- mirrors ------------------------------------------------------------------------------------------------------------
def test_python_mirror_checks_before_the_device():
    p = _params()
    key = P.SecretKey(p, np.zeros((p.k, p.l), np.int64))
    parties = [P.Party(i, key) for i in range(p.n)]
    ones = lambda c: [1] * len(c)
    for fn in (lambda c, w, **kw: P.combine_ciphertexts(c, w, **kw), lambda c, w, **kw: P.decrypt_party_combination(c, w, key, 0, **kw),
               lambda c, w, **kw: P.decrypt_all_party_combinations(c, w, parties, **kw)):
        with pytest.raises(P.PvwError, match="No ciphertexts provided"):
            fn([], [])
        bad = _cts(p, 3)
        bad[2] = P.PvwCiphertext(np.zeros((p.k - 1, p.L, p.l), np.uint64), bad[2].c2, p, P.REPR_NTT)
        with pytest.raises(P.PvwError, match="DimensionMismatch: Ciphertext 2"):
            fn(bad, ones(bad))
        with pytest.raises(P.PvwError, match="DimensionMismatch: Ciphertext 1 is in representation"):
            fn([_cts(p, 1)[0], _cts(p, 1, P.REPR_POWER)[0]], [1, 1])
        with pytest.raises(P.PvwError, match="DimensionMismatch: valid"):
            fn(_cts(p, 3), [1, 1, 1], valid=[1, 0])
        with pytest.raises(P.PvwError, match="DimensionMismatch: weights: expected 3 weights, got 2"):
            fn(_cts(p, 3), [1, 1])
        for w in ([1, 1 << 63, 1], [1, -(1 << 63) - 1, 1]):
            with pytest.raises(P.PvwError, match="outside the int64 range"):
                fn(_cts(p, 3), w)
        with pytest.raises(P.PvwError, match="InsufficientData: No valid dealer"):
            fn(_cts(p, 3), [1, 1, 1], valid=[0, 0, 0])
        with pytest.raises(P.PvwError, match="InsufficientData: No participating dealer"):
            fn(_cts(p, 3), [0, 5, 0], valid=[1, 0, 1])
    with pytest.raises(P.PvwError, match=f"Party index {p.n} exceeds maximum {p.n - 1}"):
        P.decrypt_party_combination(_cts(p, 2), [1, 1], key, p.n)
    with pytest.raises(P.PvwError, match="consecutive"):
        P.decrypt_all_party_combinations(_cts(p, 2), [1, 1], [parties[0], parties[2]])
    assert P.decrypt_all_party_combinations(_cts(p, 2), [1, 1], []).values.shape == (0,)
    with pytest.raises(P.PvwError, match="DimensionMismatch: valid"):
        p.lincomb_fits([1, 2, 3], [1, 0])
    # the host form of the combination runs without a device and keeps parameters and representation
    rng = np.random.default_rng(3)
    cts = [P.PvwCiphertext(rng.integers(0, 1 << 64, (p.k, p.L, p.l), dtype=np.uint64),
                           rng.integers(0, 1 << 64, (p.n, p.L, p.l), dtype=np.uint64), p, P.REPR_POWER) for _ in range(4)]
    w = [I64_MIN, 3, -7, I64_MAX]
    comb = P.combine_ciphertexts(cts, w, valid=[1, 1, 0, 1], host=True)
    w1, w2, _ = _restated(p, np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts]), w, [1, 1, 0, 1], 0, p.n)
    assert comb.params is p and comb.repr == P.REPR_POWER and np.array_equal(comb.c1, w1) and np.array_equal(comb.c2, w2)
    comb.validate()
    diff = P.combine_ciphertexts(cts[:2], [1, -1], host=True)       # w = -1: the difference of two ciphertexts
    q = np.array([int(x) for x in p.moduli()], dtype=object).reshape(1, -1, 1)
    assert np.array_equal(diff.c1, ((cts[0].c1.astype(object) - cts[1].c1.astype(object)) % q).astype(np.uint64))


def test_the_report_of_a_field_weighted_combination_takes_lincomb_fits_for_the_noise_test():
    from pvw_rs_amd import api
    p = _params(3, 4, 8, M.bench_moduli(17))
    lam = _lagrange_at_zero([1, 2, 3, 4, 5], PLAIN)               # residues in [0, p): field-sized
    out, noise, status = np.array([5], np.uint64), np.array([(1 << 64) - 1], np.uint64), np.zeros(1, np.uint32)
    w = np.array(lam, np.int64)
    r = api._lincomb_report(p, out, noise, status, w, None, None, True, None)
    assert r.bound == sum(abs(x) for x in lam) * p.noise_bound() >= 1 << 64 and r.valid.all()    # saturated noise, inside the radius
    small = _params(3, 4, 8, M.bench_moduli(5))
    assert not api._lincomb_report(small, out, noise, status, w, None, None, True, None).valid.any()
    r = api._lincomb_report(p, out, np.array([12], np.uint64), status, np.array([2, -3], np.int64), None, None, True, None)
    assert r.bound == 5 * p.noise_bound() and r.valid.all()
    assert not api._lincomb_report(p, out, noise, status, np.array([2, -3], np.int64), None, None, True, None).valid.any()


def test_cpp_mirror_compiles_against_the_header():
    exe = os.path.join(ROOT, "build", "ct_lincomb_cpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "ct_lincomb.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "pvw_rs_amd"), "-lpvw_hip", "-Wl,-rpath," + os.path.join(ROOT, "pvw_rs_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_rust_mirror_has_the_shims_next_to_the_sum_shims():
    src = open(os.path.join(ROOT, "rust", "pvw", "src", "crypto.rs")).read()
    for needle in ("pub fn combine(ciphertexts: &[PvwCiphertext], weights: &[i64], valid: Option<&[bool]>) -> Result<PvwCiphertext>",
                   "pub fn decrypt_combination(", "sys::pvw_ct_lincomb(", "sys::pvw_decrypt_lincomb_plain("):
        assert needle in src, needle
    assert src.index("pub fn decrypt_all_party_sums_plain(") < src.index("pub fn combine(")

"""Sums of dealers' ciphertexts on the host side: the symbols exist in both builds, pvw_ct_sum_host equals a
restatement in Python integers, the sum of model ciphertexts decrypts to the sum of the plaintexts with the noise the checked
decode reports, pvw_ctx_sum_capacity is the documented sufficient radius, argument errors come before the device, and the
mirrors check and compile.  No device compute here; the kernels are checked in tests/test_gpu_ct_sum.py."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import EXAMPLE_MODULI, MOD_TOP_56, TEST_MODULI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS, INSUFFICIENT_DATA, INVALID_FORMAT, INTERNAL = 1, 17, 18, 19
NEW = ["pvw_ct_sum_device", "pvw_ct_sum", "pvw_ct_sum_host", "pvw_decrypt_sum_checked_device", "pvw_decrypt_sum_device_sk_checked",
       "pvw_decrypt_sum_checked", "pvw_decrypt_all_sum_checked", "pvw_decrypt_all_sum_checked_device", "pvw_ctx_sum_capacity"]


def _params(n=6, k=4, l=8, moduli=TEST_MODULI):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name


def test_the_shipped_library_has_no_split_switch():
    # ... nor the staging budget of the host-buffer calls (tests/test_gpu_staged_pieces.py shrinks it in the tuning build)
    s = subprocess.run(["strings", "-a", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "PVW_SUM_SPLIT" not in s and "PVW_STAGE_BYTES" not in s
    s = subprocess.run(["strings", "-a", _ffi.LIB_TUNING_PATH], capture_output=True, text=True, check=True).stdout
    assert "PVW_SUM_SPLIT" in s and "PVW_STAGE_BYTES" in s


# ---- pvw_ct_sum_host against Python integers ------------------------------------------------------------------------
GEOMETRIES = [  # (n, k, l, moduli)
    (6, 4, 8, TEST_MODULI),
    (5, 3, 16, M.bench_moduli(1)),
    (7, 2, 32, M.bench_moduli(2)),
    (3, 5, 64, MOD_TOP_56),
    (9, 1, 8, EXAMPLE_MODULI),
    (4, 6, 16, M.bench_moduli(5)),
]


def _restated(p, c1s, c2s, valid, lo, hi):
    """out = sum over the valid dealers, word by word mod q of the word's limb, in Python integers"""
    q = np.array([int(x) for x in p.moduli()], dtype=object).reshape(1, -1, 1)
    on = [d for d in range(len(c1s)) if valid is None or valid[d]]
    c1 = sum(c1s[d].astype(object) for d in on) % q
    c2 = sum(c2s[d, lo:hi].astype(object) for d in on) % q
    return c1.astype(np.uint64), c2.astype(np.uint64)


def _host_sum(p, c1s, c2s, valid, lo, hi):
    c1 = np.zeros((p.k, p.L, p.l), np.uint64)
    c2 = np.zeros((hi - lo, p.L, p.l), np.uint64)
    cnt = C.c_uint32(77)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    rc = _ffi.lib().pvw_ct_sum_host(p._h, _ptr(c1s), _ptr(c2s), len(c1s), _ptr(v), lo, hi, _ptr(c1), _ptr(c2), C.byref(cnt))
    return rc, c1, c2, cnt.value


def _words(rng, p, D, rows, kind):
    """kind: reduced residues, any 64-bit words, or the extreme words 0, q-1, q, 2^64-1 in every position in turn"""
    q = np.array(p.moduli(), dtype=np.uint64).reshape(1, 1, -1, 1)
    shape = (D, rows, p.L, p.l)
    if kind == "reduced":
        return rng.integers(0, 1 << 62, shape, dtype=np.uint64) % q
    if kind == "any":
        return rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    pick = rng.integers(0, 4, shape)
    ext = np.stack(np.broadcast_arrays(np.uint64(0), q - np.uint64(1), q, np.uint64((1 << 64) - 1)))
    return np.ascontiguousarray(np.choose(pick, [np.broadcast_to(e, shape) for e in ext]))


@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
@pytest.mark.parametrize("D", [1, 2, 7, 130])
def test_ct_sum_host_equals_python_integers(geom, D):
    n, k, l, moduli = GEOMETRIES[geom]
    p = _params(n, k, l, moduli)
    rng = np.random.default_rng(1000 * geom + D)
    masks = [None, np.arange(D) % 2 == 0, np.arange(D) == D // 2]
    ranges = [(0, n), (1, n), (n - 1, n), (0, 1)]
    for i, kind in enumerate(["reduced", "any", "extreme"]):
        c1s, c2s = _words(rng, p, D, k, kind), _words(rng, p, D, n, kind)
        for j, valid in enumerate(masks):
            lo, hi = ranges[(i + j) % len(ranges)]
            rc, c1, c2, cnt = _host_sum(p, c1s, c2s, valid, lo, hi)
            assert rc == 0, _ffi.last_error()
            w1, w2 = _restated(p, c1s, c2s, valid, lo, hi)
            assert np.array_equal(c1, w1) and np.array_equal(c2, w2), (kind, j, lo, hi)
            assert cnt == (D if valid is None else int(np.count_nonzero(valid)))
            assert (c1 < np.array(moduli, np.uint64).reshape(1, -1, 1)).all()


def test_extreme_words_everywhere_exercise_the_carry_count():
    # 130 dealers of 2^64 - 1 in every position: the 64-bit sum wraps 129 times
    p = _params(3, 2, 8, M.bench_moduli(2))
    c1s = np.full((130, p.k, p.L, p.l), (1 << 64) - 1, np.uint64)
    c2s = np.full((130, p.n, p.L, p.l), (1 << 64) - 1, np.uint64)
    rc, c1, c2, cnt = _host_sum(p, c1s, c2s, None, 0, p.n)
    assert rc == 0 and cnt == 130
    for i, q in enumerate(int(x) for x in p.moduli()):
        assert (c1[:, i] == np.uint64(130 * ((1 << 64) - 1) % q)).all() and (c2[:, i] == np.uint64(130 * ((1 << 64) - 1) % q)).all()


def test_no_valid_dealer_is_insufficient_data():
    p = _params()
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    rc, c1, c2, cnt = _host_sum(p, c1s, c2s, np.zeros(3, np.uint8), 0, p.n)
    assert rc == INSUFFICIENT_DATA and "No valid dealer" in _ffi.last_error() and cnt == 77


# ---- homomorphism on the model ----------------------------------------------------------------------------------------
def _model_setup(moduli, n=3, k=4, l=8, seed=5):
    mp = M.Params(n, k, l, moduli, 0.5, 100, 200)
    rnd = random.Random(seed)
    A = [[[rnd.randrange(mp.Q) for _ in range(l)] for _ in range(k)] for _ in range(k)]
    sk = [[[rnd.randint(-1, 1) for _ in range(l)] for _ in range(k)] for _ in range(n)]
    B = [M.public_key(mp, A, sk[i], [[rnd.randint(-100, 100) for _ in range(l)] for _ in range(k)]) for i in range(n)]
    return mp, rnd, A, B, sk


def _model_encrypt(mp, rnd, A, B, scalars):
    k, l, n = mp.k, mp.l, mp.n
    r = [[rnd.randint(-1, 1) for _ in range(l)] for _ in range(k)]
    e1 = [[rnd.randint(-100, 100) for _ in range(l)] for _ in range(k)]
    e2 = [[rnd.randint(-200, 200) for _ in range(l)] for _ in range(n)]
    return M.encrypt(mp, A, B, scalars, r, e1, e2)


def _rns(polys, moduli):
    return np.array([M.to_rns(poly, moduli) for poly in polys], dtype=np.uint64)


@pytest.mark.parametrize("D", [1, 5, 64])
def test_the_sum_of_model_ciphertexts_decrypts_to_the_sum_of_the_plaintexts(D):
    moduli = M.bench_moduli(5)
    mp, rnd, A, B, sk = _model_setup(moduli)
    p = _params(mp.n, mp.k, mp.l, moduli)
    assert p.sum_capacity() >= 64
    shares = [[rnd.randrange(1 << 57) for _ in range(mp.n)] for _ in range(D)]
    cts = [_model_encrypt(mp, rnd, A, B, s) for s in shares]
    c1s = np.stack([_rns(c1, moduli) for c1, _ in cts])
    c2s = np.stack([_rns(c2, moduli) for _, c2 in cts])
    valid = np.array([d % 3 != 1 for d in range(D)], np.uint8) if D > 1 else None
    on = [d for d in range(D) if valid is None or valid[d]]
    rc, c1, c2, cnt = _host_sum(p, c1s, c2s, valid, 0, mp.n)
    assert rc == 0 and cnt == len(on)
    # the ring sum of the model, polynomial by polynomial
    for j in range(mp.k):
        acc = [0] * mp.l
        for d in on:
            acc = M.ring_add(acc, cts[d][0][j], mp.Q)
        assert np.array_equal(c1[j], np.array(M.to_rns(acc, moduli), np.uint64))
    sum_c1 = [M.from_rns(c1[j].tolist(), moduli) for j in range(mp.k)]
    for i in range(mp.n):
        noisy = M.decrypt_noisy(mp, sum_c1, M.from_rns(c2[i].tolist(), moduli), sk[i])
        want = sum(shares[d][i] for d in on)
        assert want < 1 << 64 and M.decode_scalar_pvw(noisy, mp) == want
        per = [P.decode_scalar_pvw_checked_host(p, _rns([M.decrypt_noisy(mp, cts[d][0], cts[d][1][i], sk[i])], moduli)) for d in on]
        assert all(int(r.values[0]) == shares[d][i] and not r.lossy[0] for r, d in zip(per, on))
        agg = P.decode_scalar_pvw_checked_host(p, _rns([noisy], moduli))
        assert int(agg.values[0]) == want and not agg.lossy[0]
        assert int(agg.noise[0]) <= sum(int(r.noise[0]) for r in per)


def test_a_sum_of_plaintexts_beyond_64_bits_is_reported_lossy():
    moduli = M.bench_moduli(5)
    mp, rnd, A, B, sk = _model_setup(moduli, seed=9)
    p = _params(mp.n, mp.k, mp.l, moduli)
    shares = [[(1 << 63) - 5 - d for _ in range(mp.n)] for d in range(3)]       # as i64: positive; the sum is >= 2^64
    cts = [_model_encrypt(mp, rnd, A, B, s) for s in shares]
    c1s = np.stack([_rns(c1, moduli) for c1, _ in cts])
    c2s = np.stack([_rns(c2, moduli) for _, c2 in cts])
    rc, c1, c2, cnt = _host_sum(p, c1s, c2s, None, 0, mp.n)
    assert rc == 0
    sum_c1 = [M.from_rns(c1[j].tolist(), moduli) for j in range(mp.k)]
    noisy = M.decrypt_noisy(mp, sum_c1, M.from_rns(c2[0].tolist(), moduli), sk[0])
    agg = P.decode_scalar_pvw_checked_host(p, _rns([noisy], moduli))
    assert agg.lossy[0] and int(agg.noise[0]) < 3 * p.noise_bound()


# ---- capacity -----------------------------------------------------------------------------------------------------------
CAPACITY = [(TEST_MODULI, 0), (EXAMPLE_MODULI, 476), (M.bench_moduli(5), 752344)]


@pytest.mark.parametrize("moduli,expected", CAPACITY)
def test_sum_capacity_is_the_sufficient_radius_over_the_noise_bound(moduli, expected):
    p = _params(32, 32, 8, moduli)
    mp = M.Params(32, 32, 8, moduli, 0.5, 100, 200)
    R = (mp.Q - 1) // (2 * (mp.delta_power_l_minus_1 + 1))
    assert R * (mp.delta_power_l_minus_1 + 1) * 2 < mp.Q <= (R + 1) * (mp.delta_power_l_minus_1 + 1) * 2
    assert p.noise_bound() == 199215
    assert p.sum_capacity() == R // p.noise_bound() == expected
    # the boundary property: any noise pattern with max |n_j| = R decodes exactly
    rnd = random.Random(R & 0xFFFF)
    for case in range(200):
        plain = rnd.randrange(1 << 64) if case % 4 else [0, 1, (1 << 64) - 1, 1 << 63][case // 4 % 4]
        noise = [rnd.choice([-R, R, rnd.randint(-R, R)]) for _ in range(mp.l)]
        noise[rnd.randrange(mp.l)] = rnd.choice([-R, R])
        z = [(-plain * mp.delta ** j + noise[j]) % mp.Q for j in range(mp.l)]
        assert M.decode_scalar_pvw(z, mp) == plain, (case, plain)
    v = C.c_uint64()
    assert _ffi.lib().pvw_ctx_sum_capacity(p._h, None) == INVALID_PARAMETERS and _ffi.lib().pvw_ctx_sum_capacity(None, C.byref(v)) == INVALID_PARAMETERS


# ---- argument errors ----------------------------------------------------------------------------------------------------
def _sum_call(lib, name, p, c1s, c2s, D, valid, lo, hi, c1, c2):
    args = [p._h, c1s, c2s, D, valid, lo, hi, c1, c2, None] + ([None] if name.endswith("_device") else [])
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", ["pvw_ct_sum", "pvw_ct_sum_device", "pvw_ct_sum_host"])
def test_ct_sum_argument_errors_come_before_the_device(name):
    lib = _ffi.lib()
    p = _params()
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    c1, c2 = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64)
    a, b, x, y = _ptr(c1s), _ptr(c2s), _ptr(c1), _ptr(c2)
    cases = [
        ((None, b, 3, 0, 6, x, y), "NULL argument"), ((a, None, 3, 0, 6, x, y), "NULL argument"),
        ((a, b, 3, 0, 6, None, y), "NULL argument"), ((a, b, 3, 0, 6, x, None), "NULL argument"),
        ((a, b, 0, 0, 6, x, y), "No ciphertexts provided"), ((a, b, 1 << 32, 0, 6, x, y), "fewer than 2^32 dealers"),
        ((a, b, 3, 2, 2, x, y), "empty row range"), ((a, b, 3, 4, 3, x, y), "row_lo > row_hi"),
        ((a, b, 3, 5, 7, x, y), "Row index 6 exceeds maximum 5"),
    ]
    for (q1, q2, D, lo, hi, o1, o2), msg in cases:
        assert _sum_call(lib, name, p, q1, q2, D, None, lo, hi, o1, o2) == INVALID_PARAMETERS, msg
        assert msg in _ffi.last_error()
    if name != "pvw_ct_sum_device":     # the host knows its mask: no valid dealer is refused before any device work
        assert _sum_call(lib, name, p, a, b, 3, _ptr(np.zeros(3, np.uint8)), 0, 6, x, y) == INSUFFICIENT_DATA
    assert not c1.any() and not c2.any()


def test_decrypt_sum_argument_errors_come_before_the_device():
    lib = _ffi.lib()
    p = _params()
    sk = np.zeros((2, p.k, p.l), np.int64)
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    out = np.zeros(2, np.uint64)
    s, a, b, o, none = _ptr(sk), _ptr(c1s), _ptr(c2s), _ptr(out), _ptr(np.zeros(3, np.uint8))
    one = lambda *x: lib.pvw_decrypt_sum_checked(p._h, *x, None, None, None)
    assert one(None, a, b, 3, None, 1, o) == INVALID_PARAMETERS and one(s, a, b, 3, None, 1, None) == INVALID_PARAMETERS
    assert one(s, a, b, 0, None, 1, o) == INVALID_PARAMETERS and "No ciphertexts provided" in _ffi.last_error()
    assert one(s, a, b, 1 << 32, None, 1, o) == INVALID_PARAMETERS and one(s, a, b, 3, None, 7, o) == INVALID_FORMAT
    assert one(s, a, b, 3, none, 1, o) == INSUFFICIENT_DATA
    dev = lambda fn, key, *x: getattr(lib, fn)(p._h, key, *x, None, None, None, None)
    for fn in ("pvw_decrypt_sum_checked_device", "pvw_decrypt_sum_device_sk_checked"):
        assert dev(fn, None, a, b, 3, None, 1, None, o) == INVALID_PARAMETERS and "NULL argument" in _ffi.last_error()
    assert dev("pvw_decrypt_sum_checked_device", s, a, b, 0, None, 1, None, o) == INVALID_PARAMETERS
    assert dev("pvw_decrypt_sum_checked_device", s, a, b, 3, None, 9, None, o) == INVALID_FORMAT
    for fn, tail in (("pvw_decrypt_all_sum_checked", [None]), ("pvw_decrypt_all_sum_checked_device", [None, None])):
        al = lambda lo, hi, *x: getattr(lib, fn)(p._h, lo, hi, *x, None, None, *tail)
        assert al(1, 3, None, a, b, 3, None, 1, o) == INVALID_PARAMETERS and al(1, 3, s, a, b, 0, None, 1, o) == INVALID_PARAMETERS
        assert al(3, 3, s, a, b, 3, None, 1, o) == INVALID_PARAMETERS and "empty party range" in _ffi.last_error()
        assert al(5, 7, s, a, b, 3, None, 1, o) == INVALID_PARAMETERS and "Party index 6 exceeds maximum 5" in _ffi.last_error()
        assert al(1, 3, s, a, b, 1 << 32, None, 1, o) == INVALID_PARAMETERS and al(1, 3, s, a, b, 3, None, 7, o) == INVALID_FORMAT
    assert lib.pvw_decrypt_all_sum_checked(p._h, 1, 3, s, a, b, 3, none, 1, o, None, None, None) == INSUFFICIENT_DATA
    assert not out.any()


@pytest.mark.skipif(P.device_available(), reason="a device is present: the calls run (tests/test_gpu_ct_sum.py)")
def test_valid_arguments_without_a_device_fail_loudly():
    lib = _ffi.lib()
    p = _params()
    sk = np.zeros((2, p.k, p.l), np.int64)
    c1s, c2s = np.zeros((3, p.k, p.L, p.l), np.uint64), np.zeros((3, p.n, p.L, p.l), np.uint64)
    c1, c2, out = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64), np.zeros(2, np.uint64)
    s, a, b, x, y, o = _ptr(sk), _ptr(c1s), _ptr(c2s), _ptr(c1), _ptr(c2), _ptr(out)
    calls = [
        lambda: lib.pvw_ct_sum(p._h, a, b, 3, None, 0, 6, x, y, None),
        lambda: lib.pvw_ct_sum_device(p._h, a, b, 3, None, 0, 6, x, y, None, None),
        lambda: lib.pvw_decrypt_sum_checked(p._h, s, a, b, 3, None, 1, o, None, None, None),
        lambda: lib.pvw_decrypt_sum_checked_device(p._h, s, a, b, 3, None, 1, None, o, None, None, None, None),
        lambda: lib.pvw_decrypt_all_sum_checked(p._h, 1, 3, s, a, b, 3, None, 1, o, None, None, None),
        lambda: lib.pvw_decrypt_all_sum_checked_device(p._h, 1, 3, s, a, b, 3, None, 1, o, None, None, None, None),
        lambda: lib.pvw_prepare(p._h, P.PREPARE_SUM, None, None),
    ]
    for call in calls:
        assert call() == INTERNAL and "no CPU fallback" in _ffi.last_error()


# ---- mirrors ------------------------------------------------------------------------------------------------------------
def _cts(p, D, repr=P.REPR_NTT):
    return [P.PvwCiphertext(np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64), p, repr) for _ in range(D)]


def test_python_mirror_checks_before_the_device():
    p = _params()
    key = P.SecretKey(p, np.zeros((p.k, p.l), np.int64))
    parties = [P.Party(i, key) for i in range(p.n)]
    for fn in (lambda c, **kw: P.aggregate_ciphertexts(c, **kw), lambda c, **kw: P.decrypt_party_sum(c, key, 0, **kw),
               lambda c, **kw: P.decrypt_all_party_sums(c, parties, **kw)):
        with pytest.raises(P.PvwError, match="No ciphertexts provided"):
            fn([])
        bad = _cts(p, 3)
        bad[2] = P.PvwCiphertext(np.zeros((p.k - 1, p.L, p.l), np.uint64), bad[2].c2, p, P.REPR_NTT)
        with pytest.raises(P.PvwError, match="DimensionMismatch: Ciphertext 2"):
            fn(bad)
        with pytest.raises(P.PvwError, match="DimensionMismatch: Ciphertext 1 is in representation"):
            fn([_cts(p, 1)[0], _cts(p, 1, P.REPR_POWER)[0]])
        with pytest.raises(P.PvwError, match="DimensionMismatch: valid"):
            fn(_cts(p, 3), valid=[1, 0])
        with pytest.raises(P.PvwError, match="InsufficientData: No valid dealer"):
            fn(_cts(p, 3), valid=[0, 0, 0])
    with pytest.raises(P.PvwError, match=f"Party index {p.n} exceeds maximum {p.n - 1}"):
        P.decrypt_party_sum(_cts(p, 2), key, p.n)
    with pytest.raises(P.PvwError, match="consecutive"):
        P.decrypt_all_party_sums(_cts(p, 2), [parties[0], parties[2]])
    assert P.decrypt_all_party_sums(_cts(p, 2), []).values.shape == (0,)
    # the host form of the aggregate runs without a device and keeps parameters and representation
    rng = np.random.default_rng(3)
    cts = [P.PvwCiphertext(rng.integers(0, 1 << 64, (p.k, p.L, p.l), dtype=np.uint64),
                           rng.integers(0, 1 << 64, (p.n, p.L, p.l), dtype=np.uint64), p, P.REPR_POWER) for _ in range(4)]
    agg = P.aggregate_ciphertexts(cts, valid=[1, 1, 0, 1], host=True)
    w1, w2 = _restated(p, np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts]), [1, 1, 0, 1], 0, p.n)
    assert agg.params is p and agg.repr == P.REPR_POWER and np.array_equal(agg.c1, w1) and np.array_equal(agg.c2, w2)
    agg.validate()


def test_cpp_mirror_compiles_against_the_header():
    exe = os.path.join(ROOT, "build", "ct_sum_cpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "ct_sum.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "pvw_rs_amd"), "-lpvw_hip", "-Wl,-rpath," + os.path.join(ROOT, "pvw_rs_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)

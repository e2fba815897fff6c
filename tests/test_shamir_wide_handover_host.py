"""Share handover over a prime field of up to 256 bits, the CPU half: the signed-digit rule, the weight rows and the
fold of the digit plaintexts against Python's own integers, the whole handover in integers (old shares re-dealt by
pvw_shamir_shares_wide_host, integer limb combinations under the weight rows, t + 1 new shares give the old secret back; the same
for a packed old sharing), the advisory fit, every refusal, the kernels' sequence as a stand-alone program under sanitizers, the
names and the mirrors.  No device is used."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from test_shamir_wide_host import CSRC, PRIMES, ROOT, SECP_N, W256, ints, params, seeds_for

LIBDIR = os.path.join(ROOT, "pvw_rs_amd")
NEW = ["pvw_shamir_wide_handover_shape", "pvw_shamir_wide_signed_digits_host", "pvw_shamir_wide_signed_digits_device",
       "pvw_shamir_wide_handover_weights_host", "pvw_shamir_wide_handover_weights_device", "pvw_shamir_wide_from_digits_host",
       "pvw_shamir_wide_from_digits_device", "pvw_decrypt_all_handover_wide", "pvw_decrypt_all_handover_wide_device",
       "pvw_ctx_wide_handover_fits"]
MIRRORS = ["shamir_wide_handover_shape", "shamir_wide_signed_digits", "shamir_wide_handover_weights", "shamir_wide_from_digits",
           "shamir_packed_wide_handover_points", "decrypt_all_party_handover_wide"]
WIDTHS = [8, 16, 31, 32, 33, 52, 60, 63, 64]


def num_digits(p, b):
    return -(-(p.bit_length() + 1) // b)


def digits_ref(x, p, b):
    """the rule of the issue in Python integers"""
    V, B = num_digits(p, b), 1 << b
    x %= p
    if x > p // 2:
        x -= p
    out = []
    for _ in range(V - 1):
        c = x % B
        if c >= B // 2:
            c -= B
        out.append(c)
        x = (x - c) // B
    return out + [x]


def weights_ref(p, indices, valid, points, limb_bits, b):
    """rows [T V][D NL] by Lagrange with pow(x, -1, p)"""
    D, NL, V = len(indices), -(-p.bit_length() // limb_bits), num_digits(p, b)
    vs = [d for d in range(D) if valid is None or valid[d]]
    pts = [0] if points is None else points
    rows = [[0] * (D * NL) for _ in range(len(pts) * V)]
    for m, pt in enumerate(pts):
        for d in vs:
            num = den = 1
            for e in vs:
                if e != d:
                    num = num * (pt - indices[e] - 1) % p
                    den = den * (indices[d] - indices[e]) % p
            lam = num * pow(den, -1, p) % p
            for w in range(NL):
                for v, c in enumerate(digits_ref(lam << (limb_bits * w), p, b)):
                    rows[m * V + v][d * NL + w] = c
    return rows


def fold_ref(p, b, wide, status):
    """wide [count][V][ww], status [count][V] -> (values, status_out)"""
    vals, sts = [], []
    for wrow, srow in zip(wide, status):
        acc, st = 0, 0
        for v, (words, s) in enumerate(zip(wrow, srow)):
            mag = sum(int(x) << (64 * k) for k, x in enumerate(words))
            acc += (-mag if int(s) & P.DEC_NEGATIVE else mag) << (b * v)
            st |= int(s)
        vals.append(acc % p)
        sts.append(st & ~P.DEC_NEGATIVE)
    return vals, sts


def edge_set(p, b):
    V, B = num_digits(p, b), 1 << b
    half = sum((B // 2) << (b * v) for v in range(V - 1))             # every low digit exactly B/2: a carry through the chain
    below = sum((B // 2 - 1) << (b * v) for v in range(V - 1))        # ... and exactly B/2 - 1: no carry anywhere
    return [0, 1, p - 1, p // 2, p // 2 + 1, p // 2 - 1, half, p - half % p, below, p - below % p, p, W256]


def test_exports_of_both_libraries_the_header_and_the_rust_block():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "pvw-hip-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert name in _ffi._SIGNATURES and ("PVW_API int32_t " + name + "(") in header and ("pub fn " + name + "(") in sys_rs, name
        for lib in ("libpvw_hip.so", "libpvw_hip_tuning.so"):
            assert hasattr(C.CDLL(os.path.join(LIBDIR, lib)), name), (lib, name)


def test_mirrors():
    hpp = open(os.path.join(ROOT, "pvw_rs_amd", "host", "pvw.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "pvw", "src", "crypto.rs")).read()
    for name in MIRRORS:
        assert name in P.__all__ and callable(getattr(P, name)), name
        assert ("inline" in hpp and name + "(" in hpp) and "pub fn " + name in rs, name
    assert hasattr(P.PvwParameters, "wide_handover_fits") and "wide_handover_fits(" in hpp and "pub fn wide_handover_fits" in rs
    assert P.shamir_packed_wide_handover_points(SECP_N, 3) == [0, SECP_N - 1, SECP_N - 2]


def test_shape():
    assert len(PRIMES) == 13
    for b in range(52, 65):
        assert P.shamir_wide_handover_shape(SECP_N, 52, b) == (5, 5)
    assert P.shamir_wide_handover_shape(2**255 - 19, 52, 64) == (5, 4)
    for p in PRIMES:
        for b in WIDTHS:
            for lb in (16, 52, 62):
                if -(-p.bit_length() // lb) <= 16:
                    assert P.shamir_wide_handover_shape(p, lb, b) == (-(-p.bit_length() // lb), num_digits(p, b))


@pytest.mark.parametrize("p", PRIMES, ids=lambda p: f"{p.bit_length()}bit")
def test_digit_rule_against_python_integers(p):
    rng = random.Random(p & 0xFFFF)
    for b in WIDTHS:
        V, B = num_digits(p, b), 1 << b
        vals = edge_set(p, b) + [rng.getrandbits(256) for _ in range(20)] + [(p // 2 + rng.randrange(-B, B)) % (1 << 256) for _ in range(8)]
        got = P.shamir_wide_signed_digits(None, vals, p, b, host=True)
        assert got.shape == (len(vals), V) and got.dtype == np.int64
        for x, row in zip(vals, got.tolist()):
            assert row == digits_ref(x, p, b), (b, hex(x))
            assert all(-(B // 2) <= c < B // 2 for c in row), (b, hex(x))
            xc = x % p if x % p <= p // 2 else x % p - p
            assert sum(c << (b * v) for v, c in enumerate(row)) == xc, (b, hex(x))


def test_the_chain_needs_the_extra_bit():
    """B = 4, V = ceil(bitlen / b) = 2, x = 6: digits 2 -> -2, then (6 + 2) / 4 = 2 is outside [-2, 2); three digits close it"""
    assert digits_ref(6, 13, 2) == [-2, -2, 1] and num_digits(13, 2) == 3 and -2 + (-2) * 4 + 16 == 6


WEIGHT_CASES = [
    # D, valid, points (None: the point 0) as functions of p and the indices
    (1, None, None),
    (2, None, None),
    (2, [0, 1], None),                                                 # one valid holder only
    (6, [1, 0, 1, 1, 1, 1], None),
    (6, [1, 0, 1, 1, 0, 1], lambda p, idx: [0, p - 1, (1 << 64) + 5 if p > (1 << 65) else p - 2]),
    (6, [1, 0, 1, 1, 1, 1], lambda p, idx: [idx[2] + 1, idx[1] + 1, 0]),     # on a valid holder, on an invalid one
    (65, None, None),
    (65, [d % 2 for d in range(65)], lambda p, idx: [0, idx[1] + 1, p - 3]),
]


@pytest.mark.parametrize("p", [65537, 2**64 + 13, 2**255 - 19, SECP_N], ids=lambda p: f"{p.bit_length()}bit")
def test_weights_against_lagrange_by_modular_inverse(p):
    rng = random.Random(p & 0xFFF)
    for D, valid, pts in WEIGHT_CASES:
        idx = rng.sample(range(min(p - 2, 200)), D)
        points = None if pts is None else pts(p, idx)
        for lb, b in ((52, 64), (62, 33), (52, 8)):
            if D == 65 and b == 8:
                continue
            got = P.shamir_wide_handover_weights(None, idx, p, valid, points, lb, b, host=True)
            want = weights_ref(p, idx, valid, points, lb, b)
            assert got.tolist() == want, (D, lb, b)
            NL, V = P.shamir_wide_handover_shape(p, lb, b)
            if valid is not None:                                      # every column of an invalid holder is 0
                for d in range(D):
                    if not valid[d]:
                        assert not got[:, d * NL:(d + 1) * NL].any()
    # a point on a valid holder is that holder's unit vector: the digits of 2^(limb_bits w) in its columns, 0 elsewhere
    idx, lb, b = [4, 7, 1], 52, 60
    NL, V = P.shamir_wide_handover_shape(p, lb, b)
    got = P.shamir_wide_handover_weights(None, idx, p, None, [8], lb, b, host=True)
    for w in range(NL):
        assert got[:, NL + w].tolist() == digits_ref(1 << (lb * w), p, b)
    assert not got[:, :NL].any() and not got[:, 2 * NL:].any()


def test_indices_up_to_two_to_the_64():
    p = 2**89 - 1
    idx = [2**64 - 1, 0, 2**63]
    got = P.shamir_wide_handover_weights(None, idx, p, None, [2**64 + 7, 0], 52, 64, host=True)
    assert got.tolist() == weights_ref(p, idx, None, [2**64 + 7, 0], 52, 64)


@pytest.mark.parametrize("p", [65537, 2**127 - 1, SECP_N, 2**256 - 189], ids=lambda p: f"{p.bit_length()}bit")
def test_fold_against_python_integers(p):
    rng = random.Random(p & 0xFF)
    for V in (1, 2, 5, 32, 33):
        for ww in (1, 2, 3, 4):
            for b in (8, 31, 32, 60, 64):
                count = 6
                wide = np.array([[[rng.getrandbits(64) for _ in range(ww)] for _ in range(V)] for _ in range(count)], dtype=np.uint64)
                status = np.array([[rng.choice([0, 1, 2, 3, 4, 6, 7]) for _ in range(V)] for _ in range(count)], dtype=np.uint32)
                wide[0] = 0                                            # zero, with and without the sign bit
                status[0, 0] = 2
                wide[1, :, 1:] = 0
                vals, st = P.shamir_wide_from_digits(None, wide, status, p, b, host=True)
                want, wst = fold_ref(p, b, wide.tolist(), status.tolist())
                assert vals == want and st.tolist() == wst, (V, ww, b)
                assert all(v < p for v in vals)
    # the status bits other than the sign pass through: truncated and lossy survive, negative does not
    vals, st = P.shamir_wide_from_digits(None, np.array([[[3], [5]]], dtype=np.uint64), np.array([[2 | 4, 1]], dtype=np.uint32), p, 16, host=True)
    assert vals == [(-3 + (5 << 16)) % p] and st.tolist() == [5]


def limbs_of(v, lb, NL):
    return [(v >> (lb * w)) & ((1 << lb) - 1) for w in range(NL)]


def lagrange_at(p, xs, pt):
    out = []
    for d, xd in enumerate(xs):
        num = den = 1
        for e, xe in enumerate(xs):
            if e != d:
                num = num * (pt - xe) % p
                den = den * (xd - xe) % p
        out.append(num * pow(den, -1, p) % p)
    return out


@pytest.mark.parametrize("b", [16, 60, 64])
def test_handover_in_integers(b):
    """the old holders re-deal their shares of a degree-2 sharing; integer limb combinations under the weight rows give every new
    party sum_d lambda_d f_d(j + 1), and t + 1 of those give the old secret back"""
    p, lb, n, t = SECP_N, 52, 12, 2
    rng = random.Random(b)
    secret = rng.randrange(p)
    old = [secret, rng.randrange(p), rng.randrange(p)]
    idx = [0, 5, 2, 7, 3, 9]
    valid = [1, 0, 1, 1, 1, 1]
    D = len(idx)
    old_shares = [sum(c * pow(i + 1, e, p) for e, c in enumerate(old)) % p for i in idx]
    redeal = ints(P.shamir_shares_wide(params(n), old_shares, t, p, seeds=seeds_for(D, tag=b), host=True))      # [D][n]
    NL, V = P.shamir_wide_handover_shape(p, lb, b)
    rows = P.shamir_wide_handover_weights(None, idx, p, valid, None, lb, b, host=True).tolist()
    vs = [d for d in range(D) if valid[d]]
    lam = dict(zip(vs, lagrange_at(p, [idx[d] + 1 for d in vs], 0)))
    new, peak = [], 0
    wide = np.zeros((n, V, 2), dtype=np.uint64)
    status = np.zeros((n, V), dtype=np.uint32)
    for j in range(n):
        limbs = [x for d in range(D) for x in limbs_of(redeal[d][j], lb, NL)]
        Pv = [sum(c * x for c, x in zip(rows[v], limbs)) for v in range(V)]
        peak = max(peak, max(abs(x).bit_length() for x in Pv))
        for v, x in enumerate(Pv):
            wide[j, v] = [abs(x) & (2**64 - 1), abs(x) >> 64]
            status[j, v] = P.DEC_NEGATIVE if x < 0 else 0
        new.append(sum(x << (b * v) for v, x in enumerate(Pv)) % p)
        assert new[-1] == sum(lam[d] * redeal[d][j] for d in vs) % p
    assert peak <= lb + b + 5 + 1 and peak <= 128                      # |P_v| < 25 2^(b-1) 2^52: the words of the decode
    vals, st = P.shamir_wide_from_digits(None, wide, status, p, b, host=True)
    assert vals == new and not st.any()
    for _ in range(3):
        pick = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct_wide(pick, [new[j] for j in pick], p) == secret


def test_handover_of_a_packed_old_sharing_in_integers():
    p, lb, b, n, t, K, told, nold = SECP_N, 52, 64, 9, 2, 3, 2, 7
    rng = random.Random(3)
    secrets = [rng.randrange(p) for _ in range(K)]
    old = ints(P.shamir_shares_packed_wide(params(nold), [secrets], K, told, p, seeds=seeds_for(1), host=True))[0]   # degree told + K - 1 = 4
    idx = [0, 1, 3, 4, 5, 6]
    valid = [1, 1, 1, 0, 1, 1]                                          # five valid holders determine degree 4
    D = len(idx)
    redeal = ints(P.shamir_shares_wide(params(n), [old[i] for i in idx], t, p, seeds=seeds_for(D, tag=9), host=True))
    points = P.shamir_packed_wide_handover_points(p, K)
    NL, V = P.shamir_wide_handover_shape(p, lb, b)
    rows = P.shamir_wide_handover_weights(None, idx, p, valid, points, lb, b, host=True).tolist()
    new = [[0] * K for _ in range(n)]
    for j in range(n):
        limbs = [x for d in range(D) for x in limbs_of(redeal[d][j], lb, NL)]
        for m in range(K):
            new[j][m] = sum(sum(c * x for c, x in zip(rows[m * V + v], limbs)) << (b * v) for v in range(V)) % p
    for m in range(K):
        pick = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct_wide(pick, [new[j][m] for j in pick], p) == secrets[m]


def test_wide_handover_fits_against_lincomb_fits():
    from _util import TEST_MODULI
    small = params(12)
    bench = P.PvwParametersBuilder().set_parties(12).set_dimension(16).set_l(8).set_moduli(M.bench_moduli(17)).build()
    assert bench.wide_handover_fits(SECP_N, 5, 52, 64) and bench.wide_handover_fits(SECP_N, 5, 52, 60)
    seen = set()
    for pr in (small, bench):
        qwords = (pr.q_total().bit_length() + 63) // 64
        for p in (65537, 2**89 - 1, SECP_N):
            for nv in (1, 5, 192, 4096):
                for lb, b in ((52, 64), (52, 60), (62, 8), (16, 33)):
                    NL = -(-p.bit_length() // lb)
                    if NL > 16:
                        continue
                    ww = -(-(lb + b + (nv * NL - 1).bit_length() + 1) // 64)
                    want = pr.lincomb_fits([-(1 << (b - 1))] * (nv * NL)) and ww <= qwords
                    assert pr.wide_handover_fits(p, nv, lb, b) == want, (p, nv, lb, b)
                    seen.add(want)
    assert seen == {True, False}


def test_refusals_of_every_entry_point():
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    pr = params(12)
    pm, even, comp = api._wide_modulus(SECP_N), api._wide_modulus(SECP_N - 1), api._wide_modulus(65537 * 65539)
    idx = np.array([0, 1, 2], dtype=np.uint64)
    dup = np.array([0, 1, 1], dtype=np.uint64)
    none = np.zeros(3, dtype=np.uint8)
    big = api._wide([SECP_N, 0])
    out = np.zeros(4096, dtype=np.int64)
    nl, nd = C.c_uint32(), C.c_uint32()
    shape = lib.pvw_shamir_wide_handover_shape
    assert shape(ptr(pm), 52, 64, C.byref(nl), C.byref(nd)) == 0
    for args in ((None, 52, 64), (ptr(even), 52, 64), (ptr(comp), 52, 64), (ptr(pm), 15, 64), (ptr(pm), 63, 64), (ptr(pm), 52, 7), (ptr(pm), 52, 65)):
        assert shape(*args, C.byref(nl), C.byref(nd)) == 1, args
    assert shape(ptr(pm), 52, 64, None, C.byref(nd)) == 1
    # signed digits: host, and the device form before any device work
    vals = api._wide([1, 2])
    for fn, head, tail in ((lib.pvw_shamir_wide_signed_digits_host, (), ()), (lib.pvw_shamir_wide_signed_digits_device, (pr._h,), (None,))):
        assert fn(*head, None, ptr(vals), 2, 64, ptr(out), *tail) == 1
        assert fn(*head, ptr(pm), None, 2, 64, ptr(out), *tail) == 1
        assert fn(*head, ptr(pm), ptr(vals), 2, 64, None, *tail) == 1
        assert fn(*head, ptr(pm), ptr(vals), 2, 7, ptr(out), *tail) == 1
        assert fn(*head, ptr(pm), ptr(vals), 2, 65, ptr(out), *tail) == 1
        assert fn(*head, ptr(even), ptr(vals), 2, 64, ptr(out), *tail) == 1
    assert lib.pvw_shamir_wide_signed_digits_device(None, ptr(pm), ptr(vals), 2, 64, ptr(out), None) == 1
    # weights
    for fn, head, tail in ((lib.pvw_shamir_wide_handover_weights_host, (), ()), (lib.pvw_shamir_wide_handover_weights_device, (pr._h,), (None,))):
        bad = [
            (None, ptr(idx), None, 3, None, 1, 52, 64, ptr(out)),
            (ptr(pm), None, None, 3, None, 1, 52, 64, ptr(out)),
            (ptr(pm), ptr(idx), None, 3, None, 1, 52, 64, None),
            (ptr(pm), ptr(idx), None, 0, None, 1, 52, 64, ptr(out)),        # no holders
            (ptr(pm), ptr(idx), None, 3, None, 0, 52, 64, ptr(out)),        # T = 0
            (ptr(pm), ptr(idx), None, 3, None, 2, 52, 64, ptr(out)),        # NULL points with T != 1
            (ptr(pm), ptr(idx), None, 3, None, 1, 52, 7, ptr(out)),
            (ptr(pm), ptr(idx), None, 3, None, 1, 52, 65, ptr(out)),
            (ptr(pm), ptr(idx), None, 3, None, 1, 15, 64, ptr(out)),
            (ptr(pm), ptr(idx), ptr(none), 3, None, 1, 52, 64, ptr(out)),   # no valid holder
            (ptr(pm), ptr(dup), None, 3, None, 1, 52, 64, ptr(out)),        # a duplicate among the valid holders
            (ptr(even), ptr(idx), None, 3, None, 1, 52, 64, ptr(out)),
            (ptr(comp), ptr(idx), None, 3, None, 1, 52, 64, ptr(out)),
            (ptr(pm), ptr(idx), None, 3, ptr(big), 2, 52, 64, ptr(out)),    # a point equal to p
            (ptr(api._wide_modulus(65537)), ptr(np.array([0, 65536], dtype=np.uint64)), None, 2, None, 1, 52, 64, ptr(out)),   # index out of range
        ]
        for args in bad:
            marker = out.copy()
            assert fn(*head, *args, *tail) == 1, (fn.__name__, args)
            assert np.array_equal(out, marker)
        # a duplicate that is masked out is no duplicate
        assert lib.pvw_shamir_wide_handover_weights_host(ptr(pm), ptr(dup), ptr(np.array([1, 1, 0], dtype=np.uint8)), 3, None, 1, 52, 64, ptr(out)) == 0
    assert lib.pvw_shamir_wide_handover_weights_device(None, ptr(pm), ptr(idx), None, 3, None, 1, 52, 64, ptr(out), None) == 1
    # the fold
    wide, st, o4, so = np.zeros((2, 5, 2), np.uint64), np.zeros((2, 5), np.uint32), np.zeros((2, 4), np.uint64), np.zeros(2, np.uint32)
    for fn, head, tail in ((lib.pvw_shamir_wide_from_digits_host, (), ()), (lib.pvw_shamir_wide_from_digits_device, (pr._h,), (None,))):
        bad = [
            (None, 64, 5, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 5, None, ptr(st), 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 5, ptr(wide), None, 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 5, ptr(wide), ptr(st), 2, 2, None, ptr(so)),
            (ptr(pm), 64, 5, ptr(wide), ptr(st), 2, 2, ptr(o4), None),
            (ptr(pm), 7, 5, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 65, 5, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 0, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 34, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 5, ptr(wide), ptr(st), 0, 2, ptr(o4), ptr(so)),
            (ptr(pm), 64, 5, ptr(wide), ptr(st), 5, 2, ptr(o4), ptr(so)),
            (ptr(even), 64, 5, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so)),
        ]
        for args in bad:
            assert fn(*head, *args, *tail) == 1, (fn.__name__, args)
    assert lib.pvw_shamir_wide_from_digits_device(None, ptr(pm), 64, 5, ptr(wide), ptr(st), 2, 2, ptr(o4), ptr(so), None) == 1
    # the handover in one call: every refusal comes before any device work (this machine has no device to reach)
    p17 = P.PvwParametersBuilder().set_parties(12).set_dimension(16).set_l(8).set_moduli(M.bench_moduli(17)).build()
    buf = np.zeros(8, dtype=np.uint64)
    idx6 = np.arange(6, dtype=np.uint64)
    for name in ("pvw_decrypt_all_handover_wide", "pvw_decrypt_all_handover_wide_device"):
        fn = getattr(lib, name)
        tail = (None,) if name.endswith("_device") else ()
        good = [p17._h, 0, 12, ptr(buf), ptr(buf), ptr(buf), 6, ptr(pm), 52, 64, ptr(idx6), None, None, 1, P.REPR_NTT, ptr(buf), ptr(buf), None]
        for pos, value in ((0, None), (3, None), (4, None), (5, None), (6, 0), (7, None), (7, ptr(even)), (8, 15), (9, 7), (9, 65), (10, None),
                           (11, ptr(np.zeros(6, dtype=np.uint8))), (13, 0), (13, 2), (15, None), (16, None), (1, 12), (2, 13)):
            args = list(good)
            args[pos] = value
            assert fn(*args, *tail) == 1, (name, pos)
        args = list(good)
        args[14] = 7                                                    # the many-combinations call's own code for a representation
        assert fn(*args, *tail) == 18, name
        # the digit plaintexts must fit the words of Q: one 36-bit modulus holds no 118-bit plaintext
        tiny = P.PvwParametersBuilder().set_parties(12).set_dimension(2).set_l(8).set_moduli(list(M.bench_moduli(17))[:1]).build()
        args = list(good)
        args[0] = tiny._h
        assert fn(*args, *tail) == 1, name
        assert "words" in _ffi.last_error(lib)
    fits = C.c_uint32()
    fit = lib.pvw_ctx_wide_handover_fits
    assert fit(pr._h, ptr(pm), 5, 52, 64, C.byref(fits)) == 0
    for args in ((None, ptr(pm), 5, 52, 64), (pr._h, None, 5, 52, 64), (pr._h, ptr(pm), 0, 52, 64), (pr._h, ptr(pm), 5, 15, 64), (pr._h, ptr(pm), 5, 52, 7),
                 (pr._h, ptr(pm), 5, 52, 65), (pr._h, ptr(even), 5, 52, 64)):
        assert fit(*args, C.byref(fits)) == 1, args
    assert fit(pr._h, ptr(pm), 5, 52, 64, None) == 1


def splitmix(state):
    while True:
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        yield z ^ (z >> 31)


def build_kernel_sequence():
    """tests/cpp/shamir_wide_handover.cpp under the address and undefined-behaviour sanitizers, as a program of its own"""
    exe = os.path.join(ROOT, "build", "shamir_wide_handover")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_wide_handover.cpp"), "-o", exe])
    return exe


def test_kernel_sequence_against_the_host_routines_under_sanitizers():
    """tests/cpp/shamir_wide_handover.cpp restates the three kernels (and the launches in front of the weights kernel) sequentially
    over pvw_wide.h, built with the address and undefined-behaviour sanitizers as a program of its own; what it prints is compared
    here with the _host routines for each of the 13 primes.  Nothing sanitized is loaded into Python."""
    out = subprocess.run([build_kernel_sequence()] + [f"{p:x}" for p in PRIMES], capture_output=True, text=True, timeout=300)
    assert len(PRIMES) == 13
    compare_kernel_sequence(out, PRIMES, [0, 2, 3, 5, 9])


def compare_kernel_sequence(out, primes, idx):
    """what the program printed for `primes` with the holders `idx` (the second masked out) against the _host routines"""
    assert out.returncode == 0 and "SHAMIR_WIDE_HANDOVER_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln[:2] in ("W ", "S ", "F ")]
    assert len(lines) == len(primes) * 4 * 3
    valid = [int(d != 1) for d in range(len(idx))]
    it = iter(lines)
    for a, p in enumerate(primes):
        state = [0x5EED0000 + a + 1]
        g = splitmix(state)
        for wi, b in enumerate((8, 33, 60, 64)):
            V = num_digits(p, b)
            w, s, f = next(it), next(it), next(it)
            assert (w[0], int(w[1]), int(w[2])) == ("W", a, b) and s[0] == "S" and f[0] == "F"
            want = P.shamir_wide_handover_weights(None, idx, p, valid, [0, idx[min(2, len(idx) - 1)] + 1, idx[1] + 1], 52, b, host=True)
            assert [int(x) for x in w[3:]] == want.reshape(-1).tolist(), (p, b)
            vals = []
            for i in range(8):
                words = [next(g), next(g), next(g)] + ([next(g)] if i < 4 else [0])
                vals.append(sum(x << (64 * k) for k, x in enumerate(words)))
            assert [int(x) for x in s[3:]] == P.shamir_wide_signed_digits(None, vals, p, b, host=True).reshape(-1).tolist(), (p, b)
            ww = 1 + wi
            wide = np.array([next(g) for _ in range(8 * V * ww)], dtype=np.uint64).reshape(8, V, ww)
            st = np.array([next(g) & 7 for _ in range(8 * V)], dtype=np.uint32).reshape(8, V)
            fv, fs = P.shamir_wide_from_digits(None, wide, st, p, b, host=True)
            assert [int(x, 16) for x in f[3::2]] == fv and [int(x) for x in f[4::2]] == fs.tolist(), (p, b)


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "shamir_wide_handover_mirror.cpp")
CPP_EXE = os.path.join(ROOT, "build", "shamir_wide_handover_cpp")


def _build_cpp():
    os.makedirs(os.path.dirname(CPP_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", CPP_SRC, "-o", CPP_EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_on_the_host():
    _build_cpp()
    out = subprocess.run([CPP_EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_HANDOVER_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

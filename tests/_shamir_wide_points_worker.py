"""Wide share repair at field points on the device: pvw_shamir_evaluate_wide_corrected_at* / _erasures_at* and
pvw_shamir_packed_wide_secrets*, bit for bit against their _host forms on values (or secrets), out, nerr, col_err and err_mask:
the points 0, 1, p - 1, p - 2, 2^64, 2^200, points on right, wrong and erased columns, duplicates and shuffles, through both sides
of the 64-point kernel-argument batch; the index device call reproduced by points = targets + 1; the point 0 equal to out; the
packed secrets against planted truth, the host form and the older Python route; point groups, secret passes and staged pieces;
hygiene; stream capture; concurrent calls; the chain deal -> aggregate -> checked decrypt-all -> mask -> fold -> packed secrets in
place.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_wide_points.py; prints SHAMIR_WIDE_POINTS_OK."""
import ctypes as C
import os
import random
import sys
import threading

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from test_shamir_wide_host import SECP_N, ints, seeds_for  # noqa: E402
from _shamir_wide_checked_worker import (DEV, INVALID_PARAMETERS, P17, P64, P255, U64, _params, dev, laid_out, nptr, ptr, same,  # noqa: E402
                                         sharing, system, u64, words)
from _shamir_wide_erasures_worker import host_erasures, pack, plans_for, plant  # noqa: E402
from _shamir_wide_evaluate_worker import device_evaluate  # noqa: E402

UNDECODABLE = P.SHAMIR_UNDECODABLE
PRIMES4 = (P17, P64, P255, SECP_N)
TS = (1, 2, 63, 64, 65, 130)                       # 64 points travel per launch of the point upload
SS = (1, 4, 5)


def host_at(idx, rows, t, pm, er, points, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape[:2]
    ix, pts = np.array(idx, dtype=np.uint64), api._wide(points)
    W = (count + 63) // 64
    val, out, nerr, col, mask = (np.full((S, len(pts), 4), 9, np.uint64), np.full((S, 4), 9, np.uint64), np.full(S, 9, np.uint32),
                                 np.full(count, 9, np.uint32), np.full((S, W), 9, np.uint64))
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_evaluate_wide_erasures_at_host(nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(er),
                                                             nptr(pts), len(pts), nptr(val), nptr(out), nptr(nerr), nptr(col), nptr(mask)), lib)
    return val, out, nerr, col, mask


class AtCall:
    """one pvw_shamir_evaluate_wide_erasures_at_device call (er None: a NULL mask) with its buffers kept; maskless=True goes
    through pvw_shamir_evaluate_wide_corrected_at_device"""

    def __init__(self, p, idx, rows, t, pm, er, points, layout="secret_major", out=True, nerr=True, col=True, mask=True, maskless=False):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm, self.maskless = p, t, api._wide_modulus(pm), maskless
        self.S, self.count = rows.shape[:2]
        self.ix, self.pts = np.array(idx, dtype=np.uint64), api._wide(points)
        self.d_sh = dev(arr)
        self.d_er = None if er is None else dev(er)
        W = (self.count + 63) // 64
        self.val = torch.full((self.S, len(self.pts), 4), -1, dtype=torch.int64, device=DEV)
        self.out = torch.full((self.S, 4), -1, dtype=torch.int64, device=DEV) if out else None
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV) if nerr else None
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV) if col else None
        self.mask = torch.full((self.S, W), -1, dtype=torch.int64, device=DEV) if mask else None

    def enqueue(self, stream_ptr):
        head = (self.p._h, nptr(self.pm), self.t, nptr(self.ix), self.count, ptr(self.d_sh), self.S, self.ss, self.ps)
        tail = (nptr(self.pts), len(self.pts), ptr(self.val), ptr(self.out), ptr(self.nerr), ptr(self.col), ptr(self.mask), stream_ptr)
        if self.maskless:
            return self.p._lib.pvw_shamir_evaluate_wide_corrected_at_device(*head, *tail)
        return self.p._lib.pvw_shamir_evaluate_wide_erasures_at_device(*head, ptr(self.d_er), *tail)

    def results(self):
        opt = lambda t_, as32=False: None if t_ is None else (t_.cpu().numpy().view(np.uint32) if as32 else u64(t_))
        return u64(self.val), opt(self.out), opt(self.nerr, True), opt(self.col, True), opt(self.mask)


def device_at(p, idx, rows, t, pm, er, points, layout, stream, **kw):
    call = AtCall(p, idx, rows, t, pm, er, points, layout, **kw)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffer_at(p, idx, rows, t, pm, er, points, layout):
    arr, _ = laid_out(rows, layout)
    val, out, nerr, col, mask = P.shamir_evaluate_wide_corrected_at(p, idx, arr, t, pm, points, layout=layout, erased=er)
    S = rows.shape[0]
    return api._wide([v for row in val for v in row]).reshape(S, len(points), 4), api._wide(out), nerr, col, mask


def points_for(idx, plans, pm, T, rng):
    """T points below pm.  0 comes first; then p - 1, 1, p - 2, 2^64 and 2^200 where below p, a point on a wrong, an erased and a
    right column, random field elements and further columns, shuffled behind the 0; the last repeats an earlier one"""
    count = len(idx)
    wrong = sorted({c for _, errs in plans for c in errs})
    gone = sorted({c for ers, _ in plans for c in ers})
    right = [c for c in range(count) if c not in wrong and c not in gone]
    pool = [pm - 1, 1, pm - 2] + [x for x in (2**64, 2**200) if x < pm]
    pool += [idx[c] + 1 for c in wrong[:2] + gone[:2] + right[:2]]
    rest = [rng.randrange(pm) for _ in range(T)] + [i + 1 for i in idx]
    rng.shuffle(rest)
    pts = (pool + rest)[:max(T - 1, 0)]
    rng.shuffle(pts)
    pts = [0] + pts
    if T > 3:
        pts[-1] = pts[1]                                            # a duplicate
    return pts[:T]


def at(tp1):
    """device == host on all five outputs at t + 1 = tp1 and r in {0, 1, 2, 3, 8}; T through {1, 2, 63, 64, 65, 130}; S through
    {1, 4, 5}; both layouts; unreduced words; with a mask (every class (eps, nu) in turn, each row its own), with a NULL mask and
    through the maskless entry point; NULL optional outputs; the host-buffer form; four primes in turn.  The first point is 0:
    its column of values is out.  points = targets + 1 reproduces the index device call."""
    N = 40
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(2500 + tp1)
    t = tp1 - 1
    k = tp1
    for r in (0, 1, 2, 3, 8):
        count = tp1 + r
        S, T, pm = SS[k % 3], TS[(k + r) % 6], PRIMES4[k % 4]
        k += 1
        idx, rows, _ = sharing(p, N, S, t, pm, count, rng, tag=k)
        plans = plans_for(S, count, r, k, rng)
        bent = plant(rows, plans, rng)
        er = pack([e for e, _ in plans], count)
        points = points_for(idx, plans, pm, T, rng)
        assert points[0] == 0 and len(points) == T
        want = host_at(idx, bent, t, pm, er, points)
        assert np.array_equal(want[0][:, 0], want[1]), ("host: the point 0 is out", tp1, r)
        assert same(want[1:], host_erasures(idx, bent, t, pm, er)), ("host: the reports are the decode's", tp1, r)
        for layout in ("secret_major", "party_major"):
            got = device_at(p, idx, bent, t, pm, er, points, layout, s)
            assert same(got, want), ("device", tp1, r, S, T, pm, layout, got[2], want[2])
            assert np.array_equal(got[0][:, 0], got[1]), ("the point 0 is out", tp1, r, layout)
        plain = host_at(idx, bent, t, pm, None, points)
        layout = ("secret_major", "party_major")[k % 2]
        assert same(device_at(p, idx, bent, t, pm, None, points, layout, s, maskless=True), plain), ("maskless", tp1, r, layout)
        assert same(device_at(p, idx, bent, t, pm, None, points, layout, s), plain), ("NULL mask", tp1, r, layout)
        assert same(buffer_at(p, idx, bent, t, pm, er, points, layout), want), ("host-buffer", tp1, r, S, T, pm, layout)
        if k % 2:
            assert same(buffer_at(p, idx, bent, t, pm, None, points, layout), plain), ("host-buffer maskless", tp1, r)
            assert same(device_at(p, idx, bent, t, pm, er, points, "secret_major", s, out=False, nerr=False), want), ("no out", tp1, r)
            assert same(device_at(p, idx, bent, t, pm, er, points, "party_major", s, col=False, mask=False), want), ("no col", tp1, r)
            got = device_at(p, idx, bent, t, pm, None, points, "secret_major", s, out=False, nerr=False, col=False, mask=False)
            assert same(got, plain), ("values alone", tp1, r)
        # the index call: targets on and off the columns, their points handed over as field elements
        targets = (list(idx) + [i for i in range(N + 3) if i not in idx])[:max(T, 2)]
        rng.shuffle(targets)
        for e in (er, None):
            old = device_evaluate(p, idx, bent, t, pm, e, targets, layout, s)
            assert same(device_at(p, idx, bent, t, pm, e, [i + 1 for i in targets], layout, s), old), ("index call", tp1, r, e is None)
        print(f"at t+1={tp1} r={r} S={S} T={T} ok", flush=True)
    print(f"at {tp1} ok", flush=True)


def far():
    """arbitrary words over p = 65537 and 257: far rows decode to polynomials nobody dealt, whose values at every field point the
    device returns as the host does; compared with _host only"""
    p = _params(7)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(2552)
    nrng = np.random.default_rng(2552)
    decoded = zero_rows = 0
    for pm in (P17, 257):
        for t, count, S in ((0, 3, 24), (1, 5, 24), (2, 6, 24)):
            r = count - t - 1
            idx = rng.sample(range(pm - 1), count)
            rows = nrng.integers(0, 2**64, (S, count, 4), dtype=np.uint64)
            er = pack([rng.sample(range(count), srow % (r + 2)) for srow in range(S)], count)
            points = [0, pm - 1] + [i + 1 for i in idx] + [rng.randrange(pm) for _ in range(4)]
            for e in (er, None):
                want = host_at(idx, rows, t, pm, e, points)
                decoded += int((want[2] != UNDECODABLE).sum())
                zero_rows += int((want[2] == UNDECODABLE).sum())
                assert same(device_at(p, idx, rows, t, pm, e, points, "secret_major", s), want), (pm, t, count, e is None)
    assert decoded > 20 and zero_rows > 20, (decoded, zero_rows)
    print("far ok", flush=True)


# ---------------------------------------------------------------------------------------------------------------- packed secrets
def packed_rows(rng, pm, N, S, t, K, count):
    """S packed rows: polynomials of degree t + K - 1 given by their coefficients, the shares of `count` random parties of N with
    every second word raised by a multiple of p, and the secrets F_s(-m)"""
    deg = t + K - 1
    polys = [[rng.randrange(pm) for _ in range(deg + 1)] for _ in range(S)]

    def f(poly, x):
        v = 0
        for a in reversed(poly):
            v = (v * x + a) % pm
        return v

    idx = rng.sample(range(N), count)
    vals = [[f(poly, i + 1) for i in idx] for poly in polys]
    vals = [[v + pm * (((1 << 256) - v) // pm) if (s_ + c) % 2 else v for c, v in enumerate(row)] for s_, row in enumerate(vals)]
    secrets = [[f(poly, pm - m) for m in range(K)] for poly in polys]
    return idx, words([v for row in vals for v in row], (S, count)), secrets


def packed_plans(rng, count, r):
    """row 0: floor(r / 2) wrong shares; row 1: r erasures; row 2: mixed; row 3: just beyond the bound, undecodable (r + 1 erasures
    at odd r and at r = 0, where every word is some polynomial's; floor(r / 2) + 1 wrong shares otherwise); row 4: clean"""
    def pick(eps, nu):
        cols = rng.sample(range(count), eps + nu)
        return sorted(cols[:eps]), sorted(cols[eps:])

    eps = r - 2 * (r // 3) if r else 0
    return [pick(0, r // 2), pick(r, 0), pick(eps, (r - eps) // 2), pick(r + 1, 0) if r % 2 or r == 0 else pick(0, r // 2 + 1), pick(0, 0)]


def host_packed(idx, rows, K, t, pm, er, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape[:2]
    ix = np.array(idx, dtype=np.uint64)
    W = (count + 63) // 64
    sec, nerr, col, mask = (np.full((S, K, 4), 9, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32),
                            np.full((S, W), 9, np.uint64))
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_packed_wide_secrets_host(nptr(api._wide_modulus(pm)), K, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(er),
                                                       nptr(sec), nptr(nerr), nptr(col), nptr(mask)), lib)
    return sec, nerr, col, mask


class PackedCall:
    """one pvw_shamir_packed_wide_secrets_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, K, t, pm, er, layout="secret_major", nerr=True, col=True, mask=True):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.K, self.t, self.pm = p, K, t, api._wide_modulus(pm)
        self.S, self.count = rows.shape[:2]
        self.ix = np.array(idx, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.d_er = None if er is None else dev(er)
        W = (self.count + 63) // 64
        self.sec = torch.full((self.S, K, 4), -1, dtype=torch.int64, device=DEV)
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV) if nerr else None
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV) if col else None
        self.mask = torch.full((self.S, W), -1, dtype=torch.int64, device=DEV) if mask else None

    def enqueue(self, stream_ptr):
        return self.p._lib.pvw_shamir_packed_wide_secrets_device(self.p._h, nptr(self.pm), self.K, self.t, nptr(self.ix), self.count,
                                                                 ptr(self.d_sh), self.S, self.ss, self.ps, ptr(self.d_er), ptr(self.sec),
                                                                 ptr(self.nerr), ptr(self.col), ptr(self.mask), stream_ptr)

    def results(self):
        opt = lambda t_, as32=False: None if t_ is None else (t_.cpu().numpy().view(np.uint32) if as32 else u64(t_))
        return u64(self.sec), opt(self.nerr, True), opt(self.col, True), opt(self.mask)


def device_packed(p, idx, rows, K, t, pm, er, layout, stream, **kw):
    call = PackedCall(p, idx, rows, K, t, pm, er, layout, **kw)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffer_packed(p, idx, rows, K, t, pm, er, layout):
    arr, _ = laid_out(rows, layout)
    sec, nerr, col, mask = P.shamir_packed_wide_secrets(p, pm, K, t, idx, arr, er, layout=layout)
    return api._wide([v for row in sec for v in row]).reshape(rows.shape[0], K, 4), nerr, col, mask


def packed(K):
    """pack = K x t in {0, 1, 4} x r in {0, 1, 2, 5} (count <= 74): floor(r / 2) wrong shares, r erasures, a mix, one row just beyond
    the bound among them, one clean row.  The device form on a [party][row] buffer in place (strides (1, S)) and on rows, the
    host-buffer form, with and without a mask: all equal the host form, the planted secrets where the errata are within the
    bound, zeros in the undecodable row, and the older Python route (corrected shares at t + K columns, then the host)"""
    N = 90
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(2600 + K)
    k = K
    for t in (0, 1, 4):
        for r in (0, 1, 2, 5):
            count = t + K + r
            pm = PRIMES4[k % 4] if K < 64 else (SECP_N, P255, P64)[k % 3]
            k += 1
            idx, rows, secrets = packed_rows(rng, pm, N, 5, t, K, count)
            plans = packed_plans(rng, count, r)
            bent = plant(rows, plans, rng)
            er = pack([e for e, _ in plans], count)
            want = host_packed(idx, bent, K, t, pm, er)
            assert want[1].tolist() == [len(plans[0][1]), 0, len(plans[2][1]), UNDECODABLE, 0], (K, t, r, want[1])
            for srow in (0, 1, 2, 4):
                assert ints(want[0][srow]) == secrets[srow], ("planted", K, t, r, srow)
            assert not want[0][3].any(), ("undecodable row", K, t, r)
            for layout in ("party_major", "secret_major"):
                assert same(device_packed(p, idx, bent, K, t, pm, er, layout, s), want), ("device", K, t, r, pm, layout)
            layout = ("secret_major", "party_major")[k % 2]
            assert same(buffer_packed(p, idx, bent, K, t, pm, er, layout), want), ("host-buffer", K, t, r, layout)
            plain = host_packed(idx, bent, K, t, pm, None)
            assert same(device_packed(p, idx, bent, K, t, pm, None, layout, s), plain), ("maskless", K, t, r, layout)
            if k % 2:
                assert same(device_packed(p, idx, bent, K, t, pm, er, layout, s, nerr=False, col=False, mask=False), want), ("secrets alone", K)
                assert same(buffer_packed(p, idx, bent, K, t, pm, None, layout), plain), ("host-buffer maskless", K, t, r)
            old = P.shamir_reconstruct_packed_wide_corrected(p, pm, K, t, idx, bent, er)
            assert [ints(row) for row in want[0]] == old[0] and same(want[1:], old[1:]), ("the older route", K, t, r)
            if K == 1:
                assert same((want[0].reshape(5, 4),) + want[1:], host_erasures(idx, bent, t, pm, er)), ("pack = 1", t, r)
            print(f"packed K={K} t={t} r={r} ok", flush=True)
    print(f"packed {K} ok", flush=True)


def groups():
    """several point groups and several secret passes at small shapes (the tuning build with small PVW_EVALUATE_GROUP_BYTES /
    PVW_CORRECT_PIECE_BYTES), the host-buffer forms through both copy paths in several staged pieces (PVW_STAGE_BYTES): all equal
    the host routines.  A group that does not start at a multiple of 64 takes its own points, the packed ones included."""
    _ffi.select("tuning")
    names = ("PVW_STAGE_BYTES", "PVW_CORRECT_PIECE_BYTES", "PVW_EVALUATE_GROUP_BYTES")
    for name in names:
        os.environ.pop(name, None)
    N, S, t, count, pm, T = 100, 23, 6, 40, SECP_N, 150
    r = count - t - 1
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(2656)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plans = plans_for(S, count, r, 0, rng)
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    points = points_for(idx, plans, pm, T, rng)
    want = host_at(idx, bent, t, pm, er, points)
    plain = host_at(idx, bent, t, pm, None, points)
    assert (want[2] == UNDECODABLE).any() and (want[2] == 0).any()
    K, tk = 20, 5                                                  # packed: count - tk - K = 15 redundant columns
    pidx, prows, _ = packed_rows(rng, pm, N, S, tk, K, count)
    pplans = plans_for(S, count, count - tk - K, 1, rng)
    pbent = plant(prows, pplans, rng)
    per = pack([e for e, _ in pplans], count)
    pwant = host_packed(pidx, pbent, K, tk, pm, per)
    assert (pwant[1] == UNDECODABLE).any() and (pwant[1] == 0).any()
    nk = r + 1
    settings = [{},
                {"PVW_EVALUATE_GROUP_BYTES": str(64 * ((count + 2 * nk + 2) * 32 + 4) + 5)},          # 64 points a group: 3 groups
                {"PVW_CORRECT_PIECE_BYTES": str(4 * ((2 * count + r + nk + 3 * T + 1) * 32 + 8) + 3)},  # 4 secrets a pass: 6 passes
                {"PVW_EVALUATE_GROUP_BYTES": str(7 * ((count + 2 * nk + 2) * 32 + 4)),                  # 7 points a group
                 "PVW_CORRECT_PIECE_BYTES": str(5 * ((2 * count + r + nk + 3 * 7 + 1) * 32 + 8))},       # and 5 secrets a pass
                {"PVW_STAGE_BYTES": str(5 * ((count + 1 + T) * 32 + 2 * 8 + 4) + 7)}]                    # 5 secrets a staged piece
    for env in settings:
        os.environ.update(env)
        try:
            for layout in ("secret_major", "party_major"):
                assert same(device_at(p, idx, bent, t, pm, er, points, layout, s), want), (env, layout)
                assert same(buffer_at(p, idx, bent, t, pm, er, points, layout), want), (env, layout)
                assert api._secret_residue(p)[0] == 0
                assert same(device_packed(p, pidx, pbent, K, tk, pm, per, layout, s), pwant), ("packed", env, layout)
                assert same(buffer_packed(p, pidx, pbent, K, tk, pm, per, layout), pwant), ("packed", env, layout)
                assert api._secret_residue(p)[0] == 0
            assert same(device_at(p, idx, bent, t, pm, None, points, "party_major", s, maskless=True), plain), env
            assert same(buffer_at(p, idx, bent, t, pm, None, points, "secret_major"), plain), env
        finally:
            for name in names:
                os.environ.pop(name, None)
    print("groups ok", flush=True)


def hygiene():
    """the secret regions are clear after a host-buffer call of either kind (and were scanned), and after a refused one, which
    writes nothing"""
    N, S, t, count, pm, T = 60, 9, 4, 30, SECP_N, 70
    p = _params(N)
    rng = random.Random(2660)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plans = plans_for(S, count, count - t - 1, 2, rng)
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    points = points_for(idx, plans, pm, T, rng)
    for layout in ("secret_major", "party_major"):
        assert same(buffer_at(p, idx, bent, t, pm, er, points, layout), host_at(idx, bent, t, pm, er, points)), layout
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= (2 * S * count + S + S * T) * 4, ("residue", layout, nz, scanned)
    K = 7
    pidx, prows, _ = packed_rows(rng, pm, N, S, t, K, count)
    for layout in ("secret_major", "party_major"):
        assert same(buffer_packed(p, pidx, prows, K, t, pm, er, layout), host_packed(pidx, prows, K, t, pm, er)), layout
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= (2 * S * count + S + S * K) * 4, ("packed residue", layout, nz, scanned)
    pts = api._wide(points)
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    val = np.zeros((S, T, 4), np.uint64)
    rc = p._lib.pvw_shamir_evaluate_wide_erasures_at(p._h, nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(bent), S, count, 1, nptr(er),
                                                     nptr(pts), T, nptr(val), None, None, None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib) and not val.any()
    pts[5] = api._wide([pm])[0]
    rc = p._lib.pvw_shamir_evaluate_wide_erasures_at(p._h, nptr(api._wide_modulus(pm)), t, nptr(np.array(idx, dtype=np.uint64)), count,
                                                     nptr(bent), S, count, 1, nptr(er), nptr(pts), T, nptr(val), None, None, None, None)
    assert rc == INVALID_PARAMETERS and "point out of range" in _ffi.last_error(p._lib) and not val.any()
    sec = np.zeros((S, K, 4), np.uint64)
    rc = p._lib.pvw_shamir_packed_wide_secrets(p._h, nptr(api._wide_modulus(pm)), K, t, nptr(ix), count, nptr(prows), S, count, 1, nptr(er),
                                               nptr(sec), None, None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib) and not sec.any()
    assert api._secret_residue(p)[0] == 0
    print("hygiene ok", flush=True)


def capture():
    """under stream capture the packed _device call is refused with its own error on a stream nothing has sized and on one sized
    without a mask when it has one, and the capture survives empty; after sizing, ONE captured call replays twice with other
    shares and another mask: it takes no host array of points"""
    N, S, t, K, count, pm = 90, 9, 10, 6, 60, SECP_N
    r = count - t - K
    rng = random.Random(2657)
    p = _params(N)
    idx, rows, _ = packed_rows(rng, pm, N, S, t, K, count)
    plans = plans_for(S, count, r, 1, rng)
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    want = host_packed(idx, bent, K, t, pm, er)
    call = PackedCall(p, idx, bent, K, t, pm, er)
    unmasked = PackedCall(p, idx, bent, K, t, pm, None)

    def refused(stream, what):
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=stream):
            rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
            msg = _ffi.last_error(p._lib)
        torch.cuda.synchronize()
        assert rc == INVALID_PARAMETERS and "capture" in msg and "packed wide secrets" in msg, (what, rc, msg)
        sec, nerr, col, mask = call.results()                      # nothing was enqueued: the buffers keep their fill
        assert (sec == np.uint64(U64)).all() and (nerr == 9).all() and (col == 9).all() and (mask == np.uint64(U64)).all(), what
        del g0

    torch.cuda.synchronize()
    s0 = torch.cuda.Stream(device=DEV)
    refused(s0, "unsized")                                         # a fresh context: refused before its device is touched
    api._check(unmasked.enqueue(C.c_void_p(s0.cuda_stream)), p._lib)   # sizes the stream's workspace for the maskless call only
    s0.synchronize()
    assert same(unmasked.results(), host_packed(idx, bent, K, t, pm, None))
    refused(s0, "sized without a mask")
    s1 = torch.cuda.Stream(device=DEV)
    api._check(call.enqueue(C.c_void_p(s1.cuda_stream)), p._lib)
    s1.synchronize()
    assert same(call.results(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s1):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    api._check(rc, p._lib)
    for rep in range(2):
        plans2 = plans_for(S, count, r, 2 + 3 * rep, rng)
        er2 = pack([e for e, _ in plans2], count)
        deg = t + K - 1                                            # the same parties, fresh polynomials
        polys = [[rng.randrange(pm) for _ in range(deg + 1)] for _ in range(S)]
        vals = [[sum(a * pow(i + 1, j, pm) for j, a in enumerate(poly)) % pm for i in idx] for poly in polys]
        mine = plant(words([v for row in vals for v in row], (S, count)), plans2, rng)
        call.d_sh.copy_(dev(mine))
        call.d_er.copy_(dev(er2))
        call.sec.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_packed(idx, mine, K, t, pm, er2)
        assert (want2[1] == UNDECODABLE).any() and (want2[1] != UNDECODABLE).any() and not np.array_equal(er2, er)
        assert same(call.results(), want2), rep
    del g
    print("capture ok", flush=True)


def concurrent():
    """two threads on one context overlap host-buffer calls of both kinds and of different shapes: every result equals the serial
    one bit for bit, nothing is left in a workspace"""
    N = 90
    p = _params(N)
    rng = random.Random(2658)
    jobs = []
    for k, (S, t, count, pm, T) in enumerate(((5, 4, 12, SECP_N, 9), (12, 10, 50, P255, 65), (7, 9, 40, P64, 30), (12, 3, 30, P17, 4))):
        layout = ("secret_major", "party_major")[k % 2]
        if k % 2:
            K = min(T, count - t - 4)
            idx, rows, _ = packed_rows(rng, pm, N, S, t, K, count)
            plans = plans_for(S, count, count - t - K, k, rng)
            bent = plant(rows, plans, rng)
            er = pack([e for e, _ in plans], count)
            jobs.append(lambda idx=idx, bent=bent, K=K, t=t, pm=pm, er=er, layout=layout: buffer_packed(p, idx, bent, K, t, pm, er, layout))
        else:
            idx, rows, _ = sharing(p, N, S, t, pm, count, rng, tag=k)
            plans = plans_for(S, count, count - t - 1, k, rng)
            bent = plant(rows, plans, rng)
            er = pack([e for e, _ in plans], count) if k else None
            points = points_for(idx, plans, pm, T, rng)
            jobs.append(lambda idx=idx, bent=bent, t=t, pm=pm, er=er, points=points, layout=layout:
                        buffer_at(p, idx, bent, t, pm, er, points, layout))
    serial = [job() for job in jobs]
    assert api._secret_residue(p)[0] == 0
    rounds, nthreads = 4, 2
    start = threading.Barrier(nthreads)
    failures = []

    def work(me):
        try:
            start.wait()
            for rnd in range(rounds):
                j = (2 * rnd + me) % len(jobs)
                if not same(jobs[j](), serial[j]):
                    failures.append((me, rnd, j))
        except Exception as e:  # noqa: BLE001
            failures.append((me, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures, failures
    assert api._secret_residue(p)[0] == 0
    print("concurrent ok", flush=True)


def loop():
    """the loop closed on the device over the secp256k1 order at n = 12, t = 3, K = 3, five dealers: deal
    (deal_party_shares_packed_wide) -> the dealers' ciphertexts summed limb by limb (aggregate_ciphertexts) -> the checked
    decrypt-all of the NL sums, [party][w] -> pvw_shamir_wide_erasure_mask_device on that report in place -> the fold in place ->
    pvw_shamir_packed_wide_secrets_device in place: sum_d s_{d,j} mod p for every j.  Clean; with two parties' sums overwritten (c2
    of limb 0 moved by another scalar's encoding: a clean report, another value); and with one of the two flagged instead (a
    saturated noise)."""
    rng = random.Random(2661)
    n, k, l, D, t, K, pm, lb = 12, 16, 8, 5, 3, 3, SECP_N, 52
    p, gpk, parties = system(n, k, l, M.bench_moduli(17))
    nl = P.shamir_wide_limbs(pm, lb)
    secrets = [[pm - 1 - rng.randrange(1 << 100) for _ in range(K)] for _ in range(D)]
    cts = P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, seeds=seeds_for(D * nl, tag=25), limb_bits=lb)
    want = [sum(secrets[d][j] for d in range(D)) % pm for j in range(K)]
    quiet = p.encode_scalar(777, P.REPR_NTT).astype(object)
    e = np.zeros((p.L, p.l), dtype=np.uint64)
    e[:, 1] = [(1 << 70) % q for q in p.moduli()]
    loud = p.ntt_forward(e).astype(object) + quiet
    qq = np.array(p.moduli(), dtype=object)[:, None]
    a, b = sorted(rng.sample(range(n), 2))
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    pmw = api._wide_modulus(pm)
    d_sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
    idx = np.arange(n, dtype=np.uint64)
    for run, (moved, flagged) in enumerate((((), ()), ((a, b), ()), ((a,), (b,)))):
        sums = [P.aggregate_ciphertexts([cts[d][w] for d in range(D)]) for w in range(nl)]
        assert sums[0].repr == P.REPR_NTT
        for party in moved:
            sums[0].c2[party] = ((sums[0].c2[party].astype(object) + quiet) % qq).astype(np.uint64)
        for party in flagged:
            sums[1].c2[party] = ((sums[1].c2[party].astype(object) + loud) % qq).astype(np.uint64)
        c1, c2 = dev(np.stack([c.c1 for c in sums])), dev(np.stack([c.c2 for c in sums]))
        limbs = torch.zeros((n, nl), dtype=torch.int64, device=DEV)
        noise = torch.zeros((n, nl), dtype=torch.int64, device=DEV)
        status = torch.zeros((n, nl), dtype=torch.int32, device=DEV)
        d_mask = torch.full((1, 1), 5, dtype=torch.int64, device=DEV)
        sec = torch.full((1, K, 4), -1, dtype=torch.int64, device=DEV)
        nerr = torch.full((1,), 9, dtype=torch.int32, device=DEV)
        col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
        emask = torch.full((1, 1), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        p._call("pvw_decrypt_all_checked_device", 0, n, ptr(d_sk), ptr(c1), ptr(c2), nl, sums[0].repr, ptr(limbs), ptr(noise), ptr(status), sp)
        p._call("pvw_shamir_wide_erasure_mask_device", ptr(status), ptr(noise), P.DEC_LOSSY, p.noise_bound(), n, 1, nl, nl, nl, 1, ptr(d_mask), sp)
        folded = P.shamir_wide_from_limbs_device(p, limbs, pm, lb, layout="limb_minor", num_limbs=nl, stream=s)   # [n][4]
        p._call("pvw_shamir_packed_wide_secrets_device", nptr(pmw), K, t, nptr(idx), n, ptr(folded), 1, 1, 1, ptr(d_mask), ptr(sec), ptr(nerr),
                ptr(col), ptr(emask), sp)
        s.synchronize()
        assert u64(d_mask).reshape(-1).tolist() == [sum(1 << i for i in flagged)], ("the checked decrypt flags exactly the loud sum", run)
        assert ints(u64(sec)[0]) == want, ("the sums of the dealers' secrets", run)
        assert nerr.cpu().tolist() == [len(moved)] and col.cpu().tolist() == [1 if i in moved else 0 for i in range(n)], run
        assert u64(emask).reshape(-1).tolist() == [sum(1 << i for i in moved)], run
        print(f"loop run {run} ok", flush=True)
    print("loop ok", flush=True)


CASES = {f.__name__: f for f in (far, groups, hygiene, capture, concurrent, loop)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("at"):
        at(int(sys.argv[1][2:]))
    elif sys.argv[1].startswith("packed"):
        packed(int(sys.argv[1][6:]))
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_POINTS_OK")

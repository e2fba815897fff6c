"""Reconstruction with erasures on the device: shamir_matmul_masked_kernel, shamir_bm_erasures_kernel, the locator
product at r + 1 terms, shamir_erasures_finish_kernel and the evaluation of 8.13 behind them, against
pvw_shamir_evaluate_erasures_host / pvw_shamir_reconstruct_erasures_host bit for bit on values, out, nerr, col_err and err_mask;
the mask builder against numpy; erased == NULL against the calls extended; the host-buffer forms (both copy paths, staged pieces,
passes, target groups, hygiene); stream capture; a full-size sharing against planted truth; the protocol loop closed; concurrent
calls on one context.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_erasures.py; prints SHAMIR_ERASURES_OK."""
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
from _shamir_correct_util import P61, P62, U64, UNDECODABLE, _basis_weights, _interpolate  # noqa: E402
from _shamir_correct_worker import (DEV, DISTINCT, INVALID_PARAMETERS, P17, _params, bend, clean_rows, dev, laid_out, nptr, ptr, same,  # noqa: E402
                                    system, unreduced)
from _shamir_correct_worker import DeviceCall as CorrectedCall  # noqa: E402
from _shamir_evaluate_worker import DeviceCall as EvaluateCall, buffers_tuple, diff  # noqa: E402
from test_shamir_host import secrets_for, seeds_for  # noqa: E402


def words_of(count):
    return (count + 63) // 64


def pack(sets, count):
    """erased column sets, one per row -> mask words [S][W]"""
    m = np.zeros((len(sets), words_of(count)), np.uint64)
    for s, cols in enumerate(sets):
        for c in cols:
            m[s, c // 64] |= np.uint64(1 << (c % 64))
    return m


def host_evaluated(idx, rows, t, pm, er, targets, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape
    ix, tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
    values = np.full((S, len(tg)), 3, np.uint64)
    out, nerr, col = np.full(S, 7, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32)
    mask = np.full((S, words_of(count)), 5, np.uint64)
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_evaluate_erasures_host(pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(er) if er is not None else None,
                                                     nptr(tg), len(tg), nptr(values), nptr(out), nptr(nerr), nptr(col), nptr(mask)), lib)
    return values, out, nerr, col, mask


def host_tiled(idx, rows, t, pm, er, targets):
    """the host routine's report on rows (and mask rows) whose row s repeats row s % DISTINCT: the distinct rows are decoded once"""
    S = rows.shape[0]
    if S <= DISTINCT:
        return host_evaluated(idx, rows, t, pm, er, targets)
    assert all(np.array_equal(rows[s], rows[s % DISTINCT]) and np.array_equal(er[s], er[s % DISTINCT]) for s in range(DISTINCT, S))
    values, out, nerr, _, mask = host_evaluated(idx, rows[:DISTINCT], t, pm, er[:DISTINCT], targets)
    pick = np.arange(S) % DISTINCT
    values, out, nerr, mask = values[pick], out[pick], nerr[pick], mask[pick]
    col = np.zeros(rows.shape[1], np.uint32)
    for c in range(rows.shape[1]):
        col[c] = int(((mask[:, c // 64] >> np.uint64(c % 64)) & np.uint64(1)).sum())
    return values, out, nerr, col, mask


class DeviceCall:
    """one pvw_shamir_evaluate_erasures_device call (targets given) or pvw_shamir_reconstruct_erasures_device call, its buffers kept"""

    def __init__(self, p, idx, rows, t, pm, er, targets=None, layout="secret_major"):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, pm
        self.S, self.count = rows.shape
        self.ix = np.array(idx, dtype=np.uint64)
        self.tg = None if targets is None else np.array(targets, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.d_er = None if er is None else dev(er)
        self.refill()

    def refill(self):
        self.values = torch.full((self.S, 1 if self.tg is None else len(self.tg)), 3, dtype=torch.int64, device=DEV)
        self.out = torch.full((self.S,), -1, dtype=torch.int64, device=DEV)
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV)
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV)
        self.mask = torch.full((self.S, words_of(self.count)), 5, dtype=torch.int64, device=DEV)

    def enqueue(self, stream_ptr):
        head = (self.p._h, self.pm, self.t, nptr(self.ix), self.count, ptr(self.d_sh), self.S, self.ss, self.ps, ptr(self.d_er))
        tail = (ptr(self.out), ptr(self.nerr), ptr(self.col), ptr(self.mask), stream_ptr)
        if self.tg is None:
            return self.p._lib.pvw_shamir_reconstruct_erasures_device(*head, *tail)
        return self.p._lib.pvw_shamir_evaluate_erasures_device(*head, nptr(self.tg), len(self.tg), ptr(self.values), *tail)

    def results(self):
        rest = (self.out.cpu().numpy().view(np.uint64), self.nerr.cpu().numpy().view(np.uint32), self.col.cpu().numpy().view(np.uint32),
                self.mask.cpu().numpy().view(np.uint64))
        return rest if self.tg is None else (self.values.cpu().numpy().view(np.uint64),) + rest


def device_run(p, idx, rows, t, pm, er, targets, layout, stream):
    call = DeviceCall(p, idx, rows, t, pm, er, targets, layout)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffers_run(p, idx, rows, t, pm, er, targets, layout):
    arr, _ = laid_out(rows, layout)
    if targets is None:
        return buffers_tuple(P.shamir_reconstruct_corrected(p, idx, arr.tolist(), t, pm, layout=layout, erased=er))
    return buffers_tuple(P.shamir_evaluate_corrected(p, idx, arr.tolist(), t, pm, targets, layout=layout, erased=er))


def garbage(rows, sets, rng):
    """any 64-bit words at the erased positions, 2^64 - 1 among them"""
    for s, cols in enumerate(sets):
        for i, c in enumerate(sorted(cols)):
            rows[s, c] = np.uint64(U64 if i % 2 == 0 else rng.getrandbits(64))


def plan_rows(count, t, r, b, rng):
    """(erased set, wrong set) for the DISTINCT rows of matrix A at the r-th shape: row 0 nothing or one erased bit at column 0, 63, 64
    or count - 1; row 1 eps = r and no error; row 2 eps = r + 1; row 3 eps odd, so the spare column is lost, and E_s errors; row 4
    eps + 2 nu = r exactly; row 5 one error more than that.  Every third shape one whole column is erased in EVERY row of the
    matrix: it is one of each row's eps erasures, and a row planned with none erases it alone."""
    cols = list(range(count))
    whole = rng.randrange(count) if b % 3 == 1 else None

    def pick(eps, nu):
        eps = min(max(eps, int(whole is not None)), count)
        er = rng.sample(cols, eps)
        if whole is not None and whole not in er:
            er[0] = whole
        rest = [c for c in cols if c not in er]
        return set(er), set(rng.sample(rest, min(nu, len(rest))))

    single = [0, 63, 64, count - 1][b % 4]
    if whole is not None:
        single = whole
    plans = [(set(), set()) if whole is None and (b % 5 == 0 or single >= count) else ({single}, set())]
    plans.append(pick(r, 0))
    plans.append(pick(r + 1, 0))
    odd = rng.randrange(1, r + 1, 2) if r else 0            # an odd eps <= r where r >= 1
    plans.append(pick(odd, (r - odd) // 2))
    even = r - 2 * rng.randrange(r // 2 + 1)
    plans.append(pick(even, (r - even) // 2))
    plans.append(pick(even, (r - even) // 2 + 1))
    return plans


def targets_for(idx, erased, wrong, T, N, rng, pm=P61):
    """T targets over erased, wrong and right columns and other indices, with duplicates, shuffled.  The other indices lie behind
    the N parties; at p = 257 they are the few indices below p - 1 that are no column, drawn with repeats."""
    count = len(idx)
    right = [c for c in range(count) if c not in erased and c not in wrong]
    pool = [sorted(erased), sorted(wrong), right, None]
    if pm > N + 4096:
        off = rng.sample(range(N, N + 4096), T)
    else:
        free = [i for i in range(pm - 1) if i not in idx]
        off = [rng.choice(free) for _ in range(T)]
    out = []
    for j in range(T):
        kind = pool[j % 4]
        out.append(idx[kind[rng.randrange(len(kind))]] if kind else off[j])
    if T >= 3:
        out[2] = out[0]
    rng.shuffle(out)
    return out


def check_planted(want, rows, secrets, plans, idx, targets, r, pm, tag):
    """what was planted is what comes back (a false decode is about count^E / p: the small primes are left out, where a row beyond
    the bound may well lie within E_s of a polynomial nobody dealt -- there the host routine alone is the reference)"""
    if pm < (1 << 32):
        return
    for k in range(rows.shape[0]):
        er, wr = plans[k % DISTINCT]
        if len(er) + 2 * len(wr) <= r:
            assert want[1][k] == secrets[k] and want[2][k] == len(wr), (tag, k)
            assert want[4][k].tolist() == pack([wr], len(idx))[0].tolist(), (tag, k)
            for j, tg in enumerate(targets):
                if tg in idx:
                    assert want[0][k, j] == rows[k, idx.index(tg)], (tag, k, j)
        elif len(er) != r:                                 # eps = r leaves t + 1 columns: whatever they hold lies on one polynomial
            assert want[2][k] == UNDECODABLE and not want[0][k].any() and want[1][k] == 0 and not want[4][k].any(), (tag, k)


def grid(nt):
    """device == host on all five outputs at t + 1 = nt and r over the lane and block edges of the locator (r + 1 around 64 and 128),
    S and T rotating, both layouts, unreduced words, three primes, 257 among them (its sharings among 255 parties).  Matrix A:
    plan_rows.  Matrix R: per-row random masks and errors."""
    p_wide, p_small = _params(512), _params(255)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(300 + nt), np.random.default_rng(300 + nt)
    reds = (0, 1, 2, 3, 63, 64, 65, 126, 127, 128, 129, 130, 131)
    counts, widths, primes = (1, 3, 4, 5, 130), (1, 2, 63, 64, 65, 130), (P61, P62, 257)
    a = (1, 2, 5, 64, 65).index(nt)
    for b, r in enumerate(reds):
        t, count, S, T, pm = nt - 1, nt + r, counts[(a + b) % 5], widths[(a + b) % 6], primes[(a + 2 * b) % 3]
        p, N = (p_small, 255) if pm == 257 else (p_wide, 512)
        idx, secrets, rows = clean_rows(p, N, S, t, pm, count, rng, tag=a * 16 + b)
        plans_a = plan_rows(count, t, r, b, rng)
        plans_r = []
        for _ in range(DISTINCT):
            eps = rng.randrange(min(r + 2, count + 1))
            er = set(rng.sample(range(count), eps))
            rest = [c for c in range(count) if c not in er]
            nu = rng.randrange(max(r - eps, 0) // 2 + 2)
            plans_r.append((er, set(rng.sample(rest, min(nu, len(rest))))))
        for name, plans in (("A", plans_a), ("R", plans_r)):
            mat = rows.copy()
            for k in range(min(S, DISTINCT)):
                bend(mat, k, sorted(plans[k][1]), pm, rng)
            words = unreduced(mat, pm, nrng)
            garbage(words, [plans[k][0] for k in range(min(S, DISTINCT))], rng)
            for k in range(DISTINCT, S):
                words[k] = words[k % DISTINCT]
            er = pack([plans[k % DISTINCT][0] for k in range(S)], count)
            if count % 64:
                er[:, -1] |= np.uint64(U64 << (count % 64) & U64)          # padding bits set: ignored
            erased = set(c for k in range(min(S, DISTINCT)) for c in plans[k][0])
            wrong = set(c for k in range(min(S, DISTINCT)) for c in plans[k][1])
            targets = targets_for(idx, erased, wrong, T, N, rng, pm)
            want = host_tiled(idx, words, t, pm, er, targets)
            check_planted(want, rows, secrets, plans, idx, targets, r, pm, (name, nt, r))
            for layout in ("secret_major", "party_major"):
                got = device_run(p, idx, words, t, pm, er, targets, layout, s)
                assert same(got, want), (name, nt, r, S, T, pm, layout, diff(got, want))
            got = device_run(p, idx, words, t, pm, er, None, ("secret_major", "party_major")[b % 2], s)
            assert same(got, want[1:]), ("reconstruct", name, nt, r, S, pm, diff(got, want[1:]))
        print(f"grid t+1={nt} r={r} S={S} T={T} p={pm} ok", flush=True)


FAR_SHAPES = ((0, 4, 1500, 5), (0, 6, 600, 3), (1, 7, 600, 9), (1, 8, 300, 2), (2, 9, 300, 7), (4, 12, 130, 20), (63, 70, 40, 64), (64, 72, 40, 65),
              (1, 66, 30, 3), (0, 130, 12, 130))


def far_inputs(rng):
    """(t, count, S, idx, rows, mask words, targets, beyond, the host routine's report) at p = 257 for every shape: per-row random masks
    (eps in 0 .. r + 1); the even rows are arbitrary 64-bit words, the odd rows a random polynomial with E_s, E_s + 1 or E_s + 2 of
    the non-erased columns overwritten, so they sit at and just beyond the bound, where at this p another polynomial may be nearer;
    beyond[k]: row k was planted with more than E_s errors and has redundancy left (eps < r), so if it decodes, then to a polynomial
    nobody dealt"""
    pm = 257
    for t, count, S, T in FAR_SHAPES:
        r = count - t - 1
        idx = rng.sample(range(256), count)
        sets = [set(rng.sample(range(count), rng.randrange(min(r + 2, count + 1)))) for _ in range(S)]
        rows = np.array([[rng.getrandbits(64) for _ in range(count)] for _ in range(S)], dtype=np.uint64)
        beyond = np.zeros(S, dtype=bool)
        for k in range(1, S, 2):
            poly = [rng.randrange(pm) for _ in range(t + 1)]
            rest = [c for c in range(count) if c not in sets[k]]
            nu = min(max(r - len(sets[k]), 0) // 2 + rng.randrange(3), len(rest))
            hit = set(rng.sample(rest, nu))
            beyond[k] = len(sets[k]) < r and nu > (r - len(sets[k])) // 2
            for c in rest:
                if c not in hit:
                    rows[k, c] = np.uint64(sum(a * pow(idx[c] + 1, j, pm) for j, a in enumerate(poly)) % pm + pm * rng.randrange(1 << 50))
        er = pack(sets, count)
        targets = targets_for(idx, set(c for e in sets for c in e), set(), T, 255, rng, pm)
        yield t, count, S, idx, rows, er, targets, beyond, host_evaluated(idx, rows, t, pm, er, targets)


def far():
    """p = 257, arbitrary words and rows at and just beyond the bound under per-row random masks (far_inputs): many lie within E_s
    of a polynomial nobody dealt, and the device must decode them to that polynomial as the host routine does -- the far-row
    agreement of the three forms, and the one place where the Forney / Berlekamp-Massey bound and the test on the zeros of Psi_s (a
    root of Lambda_s on an erased point among them) could part from Berlekamp-Welch.  Shapes on both sides of the lane and chunk
    edges; all five outputs, both layouts, and the host-buffer form.  Some ARBITRARY rows with redundancy left (eps < r) must decode,
    some of them with errors; some rows planted beyond the bound must decode all the same, with errors; and many must not decode."""
    pm = 257
    p = _params(255)
    s = torch.cuda.Stream(device=DEV)
    arbitrary = arbitrary_with_errors = beyond_decoded = undecodable = 0
    for t, count, S, idx, rows, er, targets, beyond, want in far_inputs(random.Random(40)):
        nerr = want[2]
        eps = np.array([sum(bin(int(w)).count("1") for w in row) for row in er])
        even = np.arange(S) % 2 == 0
        arbitrary += int((even & (eps < count - t - 1) & (nerr != UNDECODABLE)).sum())
        arbitrary_with_errors += int((even & (nerr != UNDECODABLE) & (nerr > 0)).sum())
        beyond_decoded += int((beyond & (nerr != UNDECODABLE) & (nerr > 0)).sum())
        undecodable += int((nerr == UNDECODABLE).sum())
        for layout in ("secret_major", "party_major"):
            got = device_run(p, idx, rows, t, pm, er, targets, layout, s)
            assert same(got, want), ("far", t, count, S, layout, diff(got, want))
        assert same(device_run(p, idx, rows, t, pm, er, None, "secret_major", s), want[1:]), ("far reconstruct", t, count)
        assert same(buffers_run(p, idx, rows, t, pm, er, targets, "party_major"), want), ("far host-buffer", t, count)
        print(f"far t={t} count={count} S={S}: {int((nerr != UNDECODABLE).sum())} rows decode", flush=True)
    assert arbitrary > 0 and arbitrary_with_errors > 0 and beyond_decoded > 0 and undecodable > 0, (arbitrary, arbitrary_with_errors,
                                                                                                   beyond_decoded, undecodable)
    print("far ok", flush=True)


def bent_erased(p, N, S, t, pm, count, rng, nrng, tag=0):
    """rows with different erasure and error sets (eps + 2 nu below, at and above r in turn), garbage under the erasures"""
    idx, secrets, rows = clean_rows(p, N, min(S, DISTINCT), t, pm, count, rng, tag)
    r = count - t - 1
    rows = rows[[k % rows.shape[0] for k in range(S)]].copy()
    sets = []
    for k in range(S):
        eps = min(rng.randrange(r + 1), count)
        er = set(rng.sample(range(count), eps))
        rest = [c for c in range(count) if c not in er]
        nu = min(max((r - eps) // 2 + (-1, 0, 1, 0)[k % 4], 0), len(rest))
        bend(rows, k, rng.sample(rest, nu), pm, rng)
        sets.append(er)
    words = unreduced(rows, pm, nrng)
    garbage(words, sets, rng)
    return idx, words, pack(sets, count), sets


def compat():
    """erased == NULL is the existing device call, bit for bit on every output; an all-zero mask gives the same results"""
    N = 300
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    rng, nrng = random.Random(31), np.random.default_rng(31)
    from _shamir_correct_worker import bent_sharing
    for S, t, count, T, pm in ((5, 4, 12, 9, P61), (9, 20, 90, 70, P62), (4, 64, 196, 65, P17)):
        idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
        targets = targets_for(idx, set(), set(), T, N, rng)
        for layout in ("secret_major", "party_major"):
            old = EvaluateCall(p, idx, rows, t, pm, targets, layout)
            torch.cuda.synchronize()
            api._check(old.enqueue(sp), p._lib)
            s.synchronize()
            want = old.results()
            assert same(device_run(p, idx, rows, t, pm, None, targets, layout, s), want), ("NULL", S, t, count, layout)
            zero = np.zeros((S, words_of(count)), np.uint64)
            assert same(device_run(p, idx, rows, t, pm, zero, targets, layout, s), want), ("zero mask", S, t, count, layout)
            oldc = CorrectedCall(p, idx, rows, t, pm, layout)
            torch.cuda.synchronize()
            api._check(oldc.enqueue(sp), p._lib)
            s.synchronize()
            assert same(device_run(p, idx, rows, t, pm, None, None, layout, s), oldc.results()), ("NULL reconstruct", S, t, count, layout)
            assert same(buffers_run(p, idx, rows, t, pm, None, targets, layout), want)
    print("compat ok", flush=True)


def buffers():
    """the host-buffer forms == the device forms == the host routine (both copy paths); nothing that depends on the shares is left
    behind after a call, nor after a refused one"""
    N = 200
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(33), np.random.default_rng(33)
    for S, t, count, T, pm in ((1, 0, 1, 1, P17), (5, 4, 5, 9, P61), (7, 9, 77, 100, P62), (30, 64, 150, 70, P61)):
        idx, rows, er, _ = bent_erased(p, N, S, t, pm, count, rng, nrng)
        targets = targets_for(idx, set(), set(), T, N, rng)
        want = host_tiled(idx, rows, t, pm, er, targets) if S <= DISTINCT else host_evaluated(idx, rows, t, pm, er, targets)
        for layout in ("secret_major", "party_major"):
            got = buffers_run(p, idx, rows, t, pm, er, targets, layout)
            assert same(got, want), ("host-buffer", S, t, count, layout, diff(got, want))
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= 3 * S * count + 2 * S * T + S, ("residue", S, t, count, layout, nz, scanned)
            got = buffers_run(p, idx, rows, t, pm, er, None, layout)
            assert same(got, want[1:]), ("host-buffer reconstruct", S, t, count, layout)
            assert api._secret_residue(p)[0] == 0
            got = device_run(p, idx, rows, t, pm, er, targets, layout, s)
            assert same(got, want), ("device", S, t, count, layout, diff(got, want))
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= 2 * S * count + S * T, ("residue", S, t, count, layout, nz, scanned)
    ix, tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
    arr, (ss, ps) = laid_out(rows, "secret_major")
    values = np.zeros((S, T), np.uint64)
    bad_tg = tg.copy()
    bad_tg[1] = pm - 1
    rc = p._lib.pvw_shamir_evaluate_erasures(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(er), nptr(bad_tg), T, nptr(values), None, None,
                                             None, None)
    assert rc == INVALID_PARAMETERS and "target" in _ffi.last_error(p._lib) and not values.any()
    assert api._secret_residue(p)[0] == 0
    print("buffers ok", flush=True)


def pieces():
    """several pieces (the tuning build).  PVW_STAGE_BYTES: an item is (count + 1 + 2 ceil(count / 64) + T) 8 + 4 bytes with a mask.
    PVW_EVALUATE_GROUP_BYTES: (count + 2 (r + 1) + 2) 8 + 4 bytes a target.  PVW_CORRECT_PIECE_BYTES: (2 count + r + r + 1 + 3 Tg + 2) 8
    bytes a secret.  Every combination equals the host routine in both layouts, col_err summed over the pieces."""
    _ffi.select("tuning")
    N, S, t, count, T, pm = 100, 23, 6, 40, 150, P61
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(34), np.random.default_rng(34)
    idx, rows, er, _ = bent_erased(p, N, S, t, pm, count, rng, nrng)
    targets = targets_for(idx, set(), set(), T, N, rng)
    want = host_evaluated(idx, rows, t, pm, er, targets)
    assert (want[3] > 0).sum() >= 3 and (want[2] == UNDECODABLE).any() and ((want[2] != UNDECODABLE) & (want[2] > 0)).any()
    r = count - t - 1

    def check(tag):
        for layout in ("secret_major", "party_major"):
            got = buffers_run(p, idx, rows, t, pm, er, targets, layout)
            assert same(got, want), (tag, "host-buffer", layout, diff(got, want))
            assert api._secret_residue(p)[0] == 0
            got = device_run(p, idx, rows, t, pm, er, targets, layout, s)
            assert same(got, want), (tag, "device", layout, diff(got, want))
            assert same(device_run(p, idx, rows, t, pm, er, None, layout, s), want[1:]), (tag, "device reconstruct", layout)
            assert same(buffers_run(p, idx, rows, t, pm, er, None, layout), want[1:]), (tag, "host-buffer reconstruct", layout)
            assert api._secret_residue(p)[0] == 0

    item = (count + 1 + 2 + T) * 8 + 4
    group = (count + 2 * (r + 1) + 2) * 8 + 4
    secret = lambda Tg: (2 * count + r + r + 1 + 3 * Tg + 2) * 8  # noqa: E731
    settings = [
        ("stage", {"PVW_STAGE_BYTES": 5 * item + 7}),
        ("groups64", {"PVW_EVALUATE_GROUP_BYTES": 70 * group}),
        ("groups7", {"PVW_EVALUATE_GROUP_BYTES": 7 * group + 5}),
        ("passes", {"PVW_CORRECT_PIECE_BYTES": 4 * secret(T) + 3}),
        ("all", {"PVW_STAGE_BYTES": 9 * item, "PVW_EVALUATE_GROUP_BYTES": 70 * group, "PVW_CORRECT_PIECE_BYTES": 4 * secret(64) + 3}),
    ]
    for tag, env in settings:
        for k, v in env.items():
            os.environ[k] = str(v)
        try:
            check(tag)
        finally:
            for k in env:
                os.environ.pop(k, None)
        print(f"pieces {tag} ok", flush=True)
    print("pieces ok", flush=True)


def capture():
    """under stream capture in a fresh context the call is refused and the capture survives empty -- also when the stream was sized
    by the corrected evaluate call alone, whose scratch is the smaller; after one sizing call with a mask a captured call replays,
    each replay on the mask and the shares that are in the buffers then"""
    N, S, t, count, T, pm = 300, 9, 70, 200, 90, P61
    rng, nrng = random.Random(35), np.random.default_rng(35)
    p = _params(N)
    idx, rows, er, _ = bent_erased(p, N, S, t, pm, count, rng, nrng)
    targets = targets_for(idx, set(), set(), T, N, rng)
    want = host_evaluated(idx, rows, t, pm, er, targets)
    call = DeviceCall(p, idx, rows, t, pm, er, targets)
    s0 = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg, (rc, msg)
    values, out, nerr, col, mask = call.results()
    assert (values == 3).all() and (out == np.uint64(U64)).all() and (nerr == 9).all() and (col == 9).all() and (mask == 5).all()
    del g0
    # the corrected evaluate call sizes the stream for ITS scratch (E + 1 locator coefficients a row): still too small with a mask
    s1 = torch.cuda.Stream(device=DEV)
    old = EvaluateCall(p, idx, rows, t, pm, targets)
    torch.cuda.synchronize()
    api._check(old.enqueue(C.c_void_p(s1.cuda_stream)), p._lib)
    s1.synchronize()
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1, stream=s1):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg and (call.results()[0] == 3).all(), (rc, msg)
    del g1
    api._check(call.enqueue(C.c_void_p(s1.cuda_stream)), p._lib)
    s1.synchronize()
    assert same(call.results(), want), diff(call.results(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s1):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    api._check(rc, p._lib)
    for rep in range(2):
        full = P.shamir_shares(p, secrets_for(S, pm, rng), t, pm, seeds=seeds_for(S, tag=60 + rep), host=True)
        fresh = unreduced(full[:, idx], pm, nrng)          # new shares at the SAME points: the captured call carries its indices
        sets = []
        for k in range(S):
            eps = rng.randrange(count - t)
            e = set(rng.sample(range(count), eps))
            rest = [c for c in range(count) if c not in e]
            bend(fresh, k, rng.sample(rest, max((count - t - 1 - eps) // 2 + (0, 1, -1)[k % 3], 0)), pm, rng)
            sets.append(e)
        garbage(fresh, sets, rng)
        er2 = pack(sets, count)
        call.d_sh.copy_(dev(fresh))
        call.d_er.copy_(dev(er2))
        call.values.fill_(3), call.out.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_evaluated(idx, fresh, t, pm, er2, targets)
        assert (want2[2] == UNDECODABLE).any() and (want2[2] != UNDECODABLE).any()
        got = call.results()
        assert same(got, want2), (rep, diff(got, want2))
        assert api._secret_residue(p)[0] == 0
    del g
    print("capture ok", flush=True)


def mask():
    """pvw_shamir_erasure_mask_device == numpy == pvw_shamir_erasure_mask_host for both stride pairs, each NULL choice, counts on
    both sides of a word and of one wave's 64 words, and noise == noise_bound (not erased)"""
    p = _params(64)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    nrng = np.random.default_rng(36)
    lib = p._lib
    for count, S in ((1, 1), (63, 5), (64, 3), (65, 4), (130, 7), (4097, 3), (8200, 2)):
        status = nrng.integers(0, 8, size=(S, count), dtype=np.uint32)
        noise = nrng.integers(0, 100, size=(S, count), dtype=np.uint64)
        noise[0, 0] = 50
        bits, bound = 2, 50
        for layout in ("secret_major", "party_major"):
            for use_st, use_nz in ((True, True), (True, False), (False, True)):
                flag = np.zeros((S, count), bool)
                if use_st:
                    flag |= (status & bits) != 0
                if use_nz:
                    flag |= noise > bound
                want = api._erased_words(flag, S, count, "secret_major")
                st, (ss, ps) = laid_out(status, layout)
                nz, _ = laid_out(noise, layout)
                d_st, d_nz = (dev(st.view(np.int32)) if use_st else None), (dev(nz) if use_nz else None)
                d_mask = torch.full((S, words_of(count)), 5, dtype=torch.int64, device=DEV)
                torch.cuda.synchronize()
                api._check(lib.pvw_shamir_erasure_mask_device(p._h, ptr(d_st), ptr(d_nz), bits, bound, count, S, ss, ps, ptr(d_mask), sp), lib)
                s.synchronize()
                got = d_mask.cpu().numpy().view(np.uint64)
                assert np.array_equal(got, want), (count, S, layout, use_st, use_nz)
                hm = np.full((S, words_of(count)), 5, np.uint64)
                api._check(lib.pvw_shamir_erasure_mask_host(nptr(st) if use_st else None, nptr(nz) if use_nz else None, bits, bound, count, S, ss,
                                                            ps, nptr(hm)), lib)
                assert np.array_equal(hm, want)
                if use_st and use_nz:
                    t_mask = P.shamir_erasure_mask(d_st, d_nz, status_bits=bits, noise_bound=bound, layout=layout, params=p, stream=s)
                    s.synchronize()
                    assert np.array_equal(t_mask.cpu().numpy().view(np.uint64), want)
        assert not (want[0, 0] & np.uint64(1))             # the last mask is from the noise alone: noise == noise_bound does not erase
    rc = lib.pvw_shamir_erasure_mask_device(p._h, None, None, 1, 1, 4, 1, 4, 1, ptr(d_mask), sp)
    assert rc == INVALID_PARAMETERS
    print("mask ok", flush=True)


def full():
    """against planted truth, not the host routine: S = 64 sharings of degree 2047 at count = 4096 (r = 2048).  2048 erased columns
    filled with garbage return every secret and every share; 1024 erased plus 512 overwritten return the 512 as the error mask;
    one overwritten column more makes every row undecodable."""
    rng = random.Random(37)
    n, count, S, t, pm = 4160, 4096, 64, 2047, P61
    p = _params(n, 256, 8, M.bench_moduli(17))
    secrets, seeds = secrets_for(S, pm, rng), seeds_for(S)
    sd = np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()
    d_se = dev(np.array([v & U64 for v in secrets], dtype=np.uint64))
    d_sh = torch.zeros((S, n), dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    p._call("pvw_shamir_shares_device", ptr(d_se), S, t, pm, nptr(sd), None, ptr(d_sh), sp)
    s.synchronize()
    truth = d_sh.clone()
    ix, tg = np.arange(count, dtype=np.uint64), np.arange(n, dtype=np.uint64)
    values = torch.full((S, n), 3, dtype=torch.int64, device=DEV)
    out = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    nerr = torch.full((S,), 9, dtype=torch.int32, device=DEV)
    mask = torch.full((S, 64), 5, dtype=torch.int64, device=DEV)
    d_er = torch.zeros((S, 64), dtype=torch.int64, device=DEV)
    run = lambda: p._call("pvw_shamir_evaluate_erasures_device", pm, t, nptr(ix), count, ptr(d_sh), S, n, 1, ptr(d_er), nptr(tg), n,  # noqa: E731
                          ptr(values), ptr(out), ptr(nerr), None, ptr(mask), sp)
    gen = np.random.default_rng(37)
    order = rng.sample(range(count), count)
    erased = order[:2048]
    junk = torch.from_numpy(gen.integers(-(1 << 63), (1 << 63) - 1, size=(S, 2048), dtype=np.int64)).to(DEV)
    with torch.cuda.stream(s):
        d_sh[:, erased] = junk
        d_er.copy_(dev(pack([erased] * S, count)))
    run()
    s.synchronize()
    assert (nerr.cpu().numpy() == 0).all() and not mask.any().item()
    assert out.cpu().numpy().view(np.uint64).tolist() == [v % pm for v in secrets]
    assert torch.equal(values, truth), torch.nonzero(values != truth)[:4].tolist()
    # 1024 erased + 512 overwritten
    erased, wrong, extra = order[:1024], order[1024:1536], order[1536]
    bump = torch.from_numpy(gen.integers(1, pm, size=(S, 512), dtype=np.int64)).to(DEV)
    with torch.cuda.stream(s):
        d_sh.copy_(truth)
        d_sh[:, erased] = junk[:, :1024]
        d_sh[:, wrong] = (d_sh[:, wrong] + bump) % pm
        d_er.copy_(dev(pack([erased] * S, count)))
    run()
    s.synchronize()
    assert (nerr.cpu().numpy() == 512).all()
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), pack([wrong] * S, count))
    assert out.cpu().numpy().view(np.uint64).tolist() == [v % pm for v in secrets]
    assert torch.equal(values, truth), torch.nonzero(values != truth)[:4].tolist()
    with torch.cuda.stream(s):
        d_sh[:, extra] = (d_sh[:, extra] + 12345) % pm
    run()
    s.synchronize()
    assert (nerr.cpu().numpy().view(np.uint32) == UNDECODABLE).all() and not out.any().item() and not values.any().item()
    assert not mask.any().item()
    assert api._secret_residue(p)[0] == 0
    print("full ok", flush=True)


def loop():
    """the loop closed on the device (n = 24, t = 7, D = 5, p = 2^61 - 1: r = 16, E = 8): deal -> c2 of twelve (party, dealer) pairs per
    dealer tampered (another scalar's encoding and 2^70 on one coefficient added: another value, and a saturated noise in the report) ->
    pvw_decrypt_all_plain_device -> pvw_shamir_erasure_mask_device on the [party][dealer] noise and status in place (strides 1, D) ->
    pvw_shamir_evaluate_erasures_device on the [party][dealer] values in place.  Twelve bad shares a row are more than E, so the
    corrected call on the same input reports every row undecodable; as erasures (12 <= r) every secret and every tampered share
    comes back, and the share of a party that joins under index n with them."""
    rng = random.Random(38)
    n, k, l, t, D, pm = 24, 32, 8, 7, 5, P61
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    secrets = [pm - 1 - rng.randrange(1 << 20) for _ in range(D)]
    cts = P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds_for(D, tag=3))
    keys = [pt.secret_key for pt in parties]
    dealt = np.asarray(P.decrypt_many_checked(cts, keys, 0, plain_modulus=pm).values).reshape(n, D).copy()
    tampered = [sorted(rng.sample(range(n), 12)) for _ in range(D)]
    e = np.zeros((p.L, p.l), dtype=np.uint64)
    e[:, 1] = [(1 << 70) % q for q in p.moduli()]                      # saturates the noise; the encoding of 12345 moves the value
    bump = p.ntt_forward(e).astype(object) + p.encode_scalar(12345, P.REPR_NTT).astype(object)
    qq = np.array(p.moduli(), dtype=object)[:, None]
    for d, ct in enumerate(cts):
        for party in tampered[d]:
            ct.c2[party] = ((ct.c2[party].astype(object) + bump) % qq).astype(np.uint64)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    sk = dev(np.stack([kk.secret_coeffs for kk in keys]).astype(np.int64))
    c1n, c2n = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2 for c in cts]))
    d_vals = torch.zeros((n, D), dtype=torch.int64, device=DEV)
    d_noise = torch.zeros((n, D), dtype=torch.int64, device=DEV)
    d_status = torch.zeros((n, D), dtype=torch.int32, device=DEV)
    d_mask = torch.full((D, 1), 5, dtype=torch.int64, device=DEV)
    ix = np.arange(n, dtype=np.uint64)
    targets = np.array(sorted(set(c for cols in tampered for c in cols)) + [n], dtype=np.uint64)
    T = len(targets)
    values = torch.zeros((D, T), dtype=torch.int64, device=DEV)
    out = torch.zeros((D,), dtype=torch.int64, device=DEV)
    nerr = torch.full((D,), 9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p._call("pvw_decrypt_all_plain_device", 0, n, ptr(sk), ptr(c1n), ptr(c2n), D, P.REPR_NTT, ptr(d_vals), ptr(d_noise), ptr(d_status), pm, 0, None,
            sp)
    p._call("pvw_shamir_erasure_mask_device", ptr(d_status), ptr(d_noise), P.DEC_LOSSY, p.noise_bound(), n, D, 1, D, ptr(d_mask), sp)
    p._call("pvw_shamir_evaluate_erasures_device", pm, t, nptr(ix), n, ptr(d_vals), D, 1, D, ptr(d_mask), nptr(targets), T, ptr(values), ptr(out),
            ptr(nerr), None, None, sp)
    s.synchronize()
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64), pack(tampered, n)), "the checked decrypt flags exactly the tampered pairs"
    assert out.cpu().numpy().view(np.uint64).tolist() == secrets and nerr.cpu().tolist() == [0] * D
    got = values.cpu().numpy().view(np.uint64)
    vals = d_vals.cpu().numpy().view(np.uint64)
    for d in range(D):
        for j, tg in enumerate(targets[:-1]):
            assert int(got[d, j]) == int(dealt[int(tg), d]), (d, j)
        honest = [i for i in range(n) if i not in tampered[d]][:t + 1]
        bx = [i + 1 for i in honest]
        assert int(got[d, T - 1]) == _interpolate(bx, [int(dealt[i, d]) for i in honest], _basis_weights(bx, pm), n + 1, pm), d
    assert all(int(vals[i, d]) != int(dealt[i, d]) for d in range(D) for i in tampered[d]), "the tampered shares decrypt to other values"
    # the same report without the mask: 12 bad shares a row are beyond E = 8
    old = P.shamir_reconstruct_corrected(p, list(range(n)), vals.tolist(), t, pm, layout="party_major")
    assert old[1].tolist() == [UNDECODABLE] * D
    assert api._secret_residue(p)[0] == 0
    print("loop ok", flush=True)


def concurrent():
    """the promise of include/pvw_hip.h for pvw_shamir_reconstruct_erasures and pvw_shamir_evaluate_erasures: threads on one context
    overlap both calls with different shapes, every result equals the serial one bit for bit, nothing is left in a workspace"""
    N = 200
    p = _params(N)
    rng, nrng = random.Random(39), np.random.default_rng(39)
    jobs = []
    for k, (S, t, count, T, pm) in enumerate(((5, 4, 12, 9, P61), (30, 20, 90, 70, P62), (7, 9, 77, 0, P61), (12, 3, 40, 0, P17), (3, 30, 64, 130, P61),
                                              (64, 2, 9, 0, P62))):
        idx, rows, er, _ = bent_erased(p, N, S, t, pm, count, rng, nrng, tag=k)
        layout = ("secret_major", "party_major")[k % 2]
        targets = targets_for(idx, set(), set(), T, N, rng) if T else None
        jobs.append(lambda idx=idx, rows=rows, t=t, pm=pm, er=er, targets=targets, layout=layout: buffers_run(p, idx, rows, t, pm, er, targets, layout))
    serial = [job() for job in jobs]
    assert api._secret_residue(p)[0] == 0
    rounds, nthreads = 4, 6
    start = threading.Barrier(nthreads)
    failures = []

    def work(me):
        try:
            start.wait()
            for rnd in range(rounds):
                j = (me + rnd) % len(jobs)
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


CASES = {f.__name__: f for f in (far, compat, buffers, pieces, capture, mask, full, loop, concurrent)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("grid"):
        grid(int(sys.argv[1][4:]))
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_ERASURES_OK")

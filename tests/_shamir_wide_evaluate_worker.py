"""Share repair over a prime field of up to 256 bits on the device: y o M, the targets' public matrices, the three
products and the finish pass behind the wide decode, against pvw_shamir_evaluate_wide_corrected_host / _erasures_host bit for bit
on values, out, nerr, col_err and err_mask (device-pointer and host-buffer forms); a NULL mask against the maskless device call
and the reports against the decode-only device calls; far rows over small primes; target groups, passes and pieces; hygiene;
stream capture; concurrent calls; a mid-size repair against planted truth; the chain deal -> checked decrypt-all -> mask -> fold
-> repair in place.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_wide_evaluate.py; prints SHAMIR_WIDE_EVALUATE_OK."""
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
from _shamir_wide_corrected_worker import DeviceCall as CorrectedCall  # noqa: E402
from _shamir_wide_erasures_worker import DeviceCall as ErasuresCall  # noqa: E402
from _shamir_wide_erasures_worker import pack, plans_for, plant  # noqa: E402

UNDECODABLE = P.SHAMIR_UNDECODABLE
PRIMES4 = (P17, P64, P255, SECP_N)
TS = (1, 2, 31, 32, 33, 63, 64, 65, 130)
SS = (1, 3, 4, 5, 9)


def host_evaluate(idx, rows, t, pm, er, targets, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape[:2]
    ix, tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
    W = (count + 63) // 64
    val, out, nerr, col, mask = (np.full((S, len(tg), 4), 9, np.uint64), np.full((S, 4), 9, np.uint64), np.full(S, 9, np.uint32),
                                 np.full(count, 9, np.uint32), np.full((S, W), 9, np.uint64))
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_evaluate_wide_erasures_host(nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(er),
                                                          nptr(tg), len(tg), nptr(val), nptr(out), nptr(nerr), nptr(col), nptr(mask)), lib)
    return val, out, nerr, col, mask


class DeviceCall:
    """one pvw_shamir_evaluate_wide_erasures_device call (er None: a NULL mask) with its buffers kept; maskless=True goes through
    pvw_shamir_evaluate_wide_corrected_device"""

    def __init__(self, p, idx, rows, t, pm, er, targets, layout="secret_major", out=True, nerr=True, col=True, mask=True, maskless=False):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm, self.maskless = p, t, api._wide_modulus(pm), maskless
        self.S, self.count = rows.shape[:2]
        self.ix, self.tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.d_er = None if er is None else dev(er)
        W = (self.count + 63) // 64
        self.val = torch.full((self.S, len(self.tg), 4), -1, dtype=torch.int64, device=DEV)
        self.out = torch.full((self.S, 4), -1, dtype=torch.int64, device=DEV) if out else None
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV) if nerr else None
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV) if col else None
        self.mask = torch.full((self.S, W), -1, dtype=torch.int64, device=DEV) if mask else None

    def enqueue(self, stream_ptr):
        head = (self.p._h, nptr(self.pm), self.t, nptr(self.ix), self.count, ptr(self.d_sh), self.S, self.ss, self.ps)
        tail = (nptr(self.tg), len(self.tg), ptr(self.val), ptr(self.out), ptr(self.nerr), ptr(self.col), ptr(self.mask), stream_ptr)
        if self.maskless:
            return self.p._lib.pvw_shamir_evaluate_wide_corrected_device(*head, *tail)
        return self.p._lib.pvw_shamir_evaluate_wide_erasures_device(*head, ptr(self.d_er), *tail)

    def results(self):
        opt = lambda t_, as32=False: None if t_ is None else (t_.cpu().numpy().view(np.uint32) if as32 else u64(t_))
        return u64(self.val), opt(self.out), opt(self.nerr, True), opt(self.col, True), opt(self.mask)


def device_evaluate(p, idx, rows, t, pm, er, targets, layout, stream, **kw):
    call = DeviceCall(p, idx, rows, t, pm, er, targets, layout, **kw)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffer_evaluate(p, idx, rows, t, pm, er, targets, layout):
    arr, _ = laid_out(rows, layout)
    val, out, nerr, col, mask = P.shamir_evaluate_wide_corrected(p, idx, arr, t, pm, targets, layout=layout, erased=er)
    S = rows.shape[0]
    return api._wide([v for row in val for v in row]).reshape(S, len(targets), 4), api._wide(out), nerr, col, mask


def targets_for(idx, plans, N, T, rng):
    """T targets: right, wrong and erased columns, indices that are no column's (N .. and the free ones below N), a duplicate"""
    wrong = sorted({c for _, errs in plans for c in errs})
    gone = sorted({c for ers, _ in plans for c in ers})
    off = [i for i in range(N + 40) if i not in idx]
    pool = [idx[c] for c in wrong[:3] + gone[:3]] + [idx[0], off[-1], idx[-1], off[0]]
    rng.shuffle(off)
    mixed = list(idx) + off
    rng.shuffle(mixed)
    tg = (pool + mixed)[:T]
    if T > 3:
        tg[-1] = tg[0]                                              # a duplicate
    while len(tg) < T:
        tg.append(tg[len(tg) % 7])
    return tg


def small(tp1):
    """device == host on all five outputs at t + 1 = tp1 and r in {0, 1, 2, 3, 8, 9, 63, 64, 65}; T through {1, 2, 31, 32, 33, 63,
    64, 65, 130} (the tile is 64 targets x 4 secrets with the terms cut across 4 waves in chunks of 8, the inversion batch is 32);
    S through {1, 3, 4, 5, 9}; both layouts; unreduced words; with a mask (every class (eps, nu) in turn, each row its own) and
    without; junk at the erased positions, and other junk changing nothing; NULL optional outputs; four primes in turn; the
    host-buffer form"""
    N = 170
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(500 + tp1)
    t = tp1 - 1
    k = tp1
    for r in (0, 1, 2, 3, 8, 9, 63, 64, 65):
        count = tp1 + r
        S, T, pm = SS[k % 5], TS[(k + r) % 9], PRIMES4[k % 4]
        k += 1
        idx, rows, _ = sharing(p, N, S, t, pm, count, rng, tag=k)
        plans = plans_for(S, count, r, k, rng)
        bent = plant(rows, plans, rng)
        er = pack([e for e, _ in plans], count)
        targets = targets_for(idx, plans, N, T, rng)
        want = host_evaluate(idx, bent, t, pm, er, targets)
        for layout in ("secret_major", "party_major"):
            got = device_evaluate(p, idx, bent, t, pm, er, targets, layout, s)
            assert same(got, want), ("device", tp1, r, S, T, pm, layout, got[2], want[2])
        other = plant(rows, plans, random.Random(k), junk=1)      # only the junk moves
        for srow, (ers, _) in enumerate(plans):
            for c in range(count):
                if c not in ers:
                    other[srow, c] = bent[srow, c]
        assert same(device_evaluate(p, idx, other, t, pm, er, targets, "secret_major", s), want), ("junk", tp1, r)
        # without a mask: the erased positions' junk counts as errors
        plain = host_evaluate(idx, bent, t, pm, None, targets)
        layout = ("secret_major", "party_major")[k % 2]
        assert same(device_evaluate(p, idx, bent, t, pm, None, targets, layout, s, maskless=True), plain), ("maskless", tp1, r, layout)
        if k % 2 == 0 or r == 65:
            assert same(buffer_evaluate(p, idx, bent, t, pm, er, targets, layout), want), ("host-buffer", tp1, r, S, T, pm, layout)
            assert same(buffer_evaluate(p, idx, bent, t, pm, None, targets, layout), plain), ("host-buffer maskless", tp1, r)
        if k % 3 == 0:
            assert same(device_evaluate(p, idx, bent, t, pm, er, targets, "secret_major", s, out=False, nerr=False), want), ("no out", tp1, r)
            assert same(device_evaluate(p, idx, bent, t, pm, er, targets, "party_major", s, col=False, mask=False), want), ("no col", tp1, r)
            got = device_evaluate(p, idx, bent, t, pm, None, targets, "secret_major", s, out=False, nerr=False, col=False, mask=False)
            assert same(got, plain), ("values alone", tp1, r)
        print(f"small t+1={tp1} r={r} S={S} T={T} ok", flush=True)
    print(f"small {tp1} ok", flush=True)


def null():
    """a NULL mask is the maskless device call on every output; the four reports are those of the wide corrected / erasures device
    call on the same input"""
    N = 140
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(51)
    for S, t, count, pm, T in ((5, 3, 20, SECP_N, 7), (9, 32, 100, P255, 66), (2, 0, 67, P64, 33)):
        r = count - t - 1
        idx, rows, _ = sharing(p, N, S, t, pm, count, rng, tag=S)
        plans = plans_for(S, count, r, S, rng)
        bent = plant(rows, plans, rng)
        er = pack([e for e, _ in plans], count)
        targets = targets_for(idx, plans, N, T, rng)
        for layout in ("secret_major", "party_major"):
            base = device_evaluate(p, idx, bent, t, pm, None, targets, layout, s, maskless=True)
            assert same(device_evaluate(p, idx, bent, t, pm, None, targets, layout, s), base), ("NULL", S, layout)
            old = CorrectedCall(p, idx, bent, t, pm, layout)
            torch.cuda.synchronize()
            api._check(old.enqueue(C.c_void_p(s.cuda_stream)), p._lib)
            s.synchronize()
            assert same(base[1:], old.results()), ("reports, maskless", S, layout)
            masked = device_evaluate(p, idx, bent, t, pm, er, targets, layout, s)
            old = ErasuresCall(p, idx, bent, t, pm, er, layout)
            torch.cuda.synchronize()
            api._check(old.enqueue(C.c_void_p(s.cuda_stream)), p._lib)
            s.synchronize()
            assert same(masked[1:], old.results()), ("reports, mask", S, layout)
        assert same(buffer_evaluate(p, idx, bent, t, pm, None, targets, "secret_major"), base), ("host-buffer NULL", S)
    print("null ok", flush=True)


def far():
    """arbitrary words over p = 65537 and 257: far rows decode to polynomials nobody dealt, whose values the device returns as the
    host does; the rows of values of undecodable rows are 0"""
    p = _params(7)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(52)
    nrng = np.random.default_rng(52)
    decoded = zero_rows = 0
    for pm in (P17, 257):
        for t, count, S in ((0, 3, 40), (1, 5, 40), (2, 6, 40), (1, 9, 24), (3, 8, 24)):
            r = count - t - 1
            idx = rng.sample(range(pm - 1), count)
            rows = nrng.integers(0, 2**64, (S, count, 4), dtype=np.uint64)
            er = pack([rng.sample(range(count), srow % (r + 2)) for srow in range(S)], count)
            targets = list(idx) + rng.sample([i for i in range(pm - 1) if i not in idx], 5)
            rng.shuffle(targets)
            for e in (er, None):
                want = host_evaluate(idx, rows, t, pm, e, targets)
                decoded += int((want[2] != UNDECODABLE).sum())
                for srow in np.nonzero(want[2] == UNDECODABLE)[0]:
                    assert not want[0][srow].any()
                    zero_rows += 1
                for layout in ("secret_major", "party_major"):
                    assert same(device_evaluate(p, idx, rows, t, pm, e, targets, layout, s), want), (pm, t, count, layout, e is None)
    assert decoded > 40 and zero_rows > 40, (decoded, zero_rows)
    print("far ok", flush=True)


def groups():
    """several target groups and several secret passes at small shapes (the tuning build with small PVW_EVALUATE_GROUP_BYTES /
    PVW_CORRECT_PIECE_BYTES), the host-buffer form through both copy paths in several staged pieces (PVW_STAGE_BYTES): all equal
    the host routine; nothing secret is left behind after success nor after a refusal"""
    _ffi.select("tuning")
    names = ("PVW_STAGE_BYTES", "PVW_CORRECT_PIECE_BYTES", "PVW_EVALUATE_GROUP_BYTES")
    for name in names:
        os.environ.pop(name, None)
    N, S, t, count, pm, T = 100, 23, 6, 40, SECP_N, 150
    r = count - t - 1
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(56)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plans = plans_for(S, count, r, 0, rng)
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    targets = targets_for(idx, plans, N, T, rng)
    want = host_evaluate(idx, bent, t, pm, er, targets)
    plain = host_evaluate(idx, bent, t, pm, None, targets)
    assert (want[2] == UNDECODABLE).any() and (want[2] == 0).any()
    for layout in ("secret_major", "party_major"):                 # one group, one pass, one piece
        assert same(buffer_evaluate(p, idx, bent, t, pm, er, targets, layout), want), layout
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= (2 * S * count + S + S * T) * 4, ("residue", layout, nz, scanned)
    nk = r + 1
    settings = [{"PVW_EVALUATE_GROUP_BYTES": str(64 * ((count + 2 * nk + 2) * 32 + 4) + 5)},          # 64 targets a group: 3 groups
                {"PVW_CORRECT_PIECE_BYTES": str(4 * ((2 * count + r + nk + 3 * T + 1) * 32 + 8) + 3)},  # 4 secrets a pass: 6 passes
                {"PVW_EVALUATE_GROUP_BYTES": str(7 * ((count + 2 * nk + 2) * 32 + 4)),                  # 7 targets a group
                 "PVW_CORRECT_PIECE_BYTES": str(5 * ((2 * count + r + nk + 3 * 7 + 1) * 32 + 8))},       # and 5 secrets a pass
                {"PVW_STAGE_BYTES": str(5 * ((count + 1 + T) * 32 + 2 * 8 + 4) + 7)}]                    # 5 secrets a staged piece
    for env in settings:
        os.environ.update(env)
        try:
            for layout in ("secret_major", "party_major"):
                assert same(device_evaluate(p, idx, bent, t, pm, er, targets, layout, s), want), (env, layout)
                assert same(buffer_evaluate(p, idx, bent, t, pm, er, targets, layout), want), (env, layout)
                assert api._secret_residue(p)[0] == 0
            assert same(device_evaluate(p, idx, bent, t, pm, None, targets, "party_major", s, maskless=True), plain), env
            assert same(buffer_evaluate(p, idx, bent, t, pm, None, targets, "secret_major"), plain), env
        finally:
            for name in names:
                os.environ.pop(name, None)
    # a refused call leaves nothing behind and writes nothing
    tg = np.array(targets, dtype=np.uint64)
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    val = np.zeros((S, T, 4), np.uint64)
    rc = p._lib.pvw_shamir_evaluate_wide_erasures(p._h, nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(bent), S, count, 1, nptr(er),
                                                  nptr(tg), T, nptr(val), None, None, None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib) and not val.any()
    assert api._secret_residue(p)[0] == 0
    print("groups ok", flush=True)


def capture():
    """under stream capture the call is refused with its own error on a stream nothing has sized and on one sized without a mask
    when it has one, and the capture survives empty; after sizing, a captured call replays twice with other shares and another
    mask"""
    N, S, t, count, pm, T = 140, 9, 40, 110, SECP_N, 70
    r = count - t - 1
    rng = random.Random(57)
    p = _params(N)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plans = plans_for(S, count, r, 1, rng)
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    targets = targets_for(idx, plans, N, T, rng)
    want = host_evaluate(idx, bent, t, pm, er, targets)
    call = DeviceCall(p, idx, bent, t, pm, er, targets)
    unmasked = DeviceCall(p, idx, bent, t, pm, None, targets, maskless=True)

    def refused(stream, what):
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=stream):
            rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
            msg = _ffi.last_error(p._lib)
        torch.cuda.synchronize()
        assert rc == INVALID_PARAMETERS and "capture" in msg and "erasure mask" in msg, (what, rc, msg)
        val, out, nerr, col, mask = call.results()                 # nothing was enqueued: the buffers keep their fill
        assert (val == np.uint64(U64)).all() and (out == np.uint64(U64)).all() and (nerr == 9).all() and (col == 9).all(), what
        del g0

    torch.cuda.synchronize()
    s0 = torch.cuda.Stream(device=DEV)
    refused(s0, "unsized")                                         # a fresh context: refused before its device is touched
    api._check(unmasked.enqueue(C.c_void_p(s0.cuda_stream)), p._lib)   # sizes the stream's workspace for the maskless call only
    s0.synchronize()
    assert same(unmasked.results(), host_evaluate(idx, bent, t, pm, None, targets))
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
        full = P.shamir_shares_wide(p, [rng.getrandbits(256) for _ in range(S)], t, pm, seeds=seeds_for(S, tag=60 + rep), host=True)
        plans2 = plans_for(S, count, r, 2 + 3 * rep, rng)
        fresh = plant(np.ascontiguousarray(full[:, idx]), plans2, rng)
        er2 = pack([e for e, _ in plans2], count)
        call.d_sh.copy_(dev(fresh))
        call.d_er.copy_(dev(er2))
        call.val.fill_(-1), call.out.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_evaluate(idx, fresh, t, pm, er2, targets)
        assert (want2[2] == UNDECODABLE).any() and (want2[2] != UNDECODABLE).any() and not np.array_equal(er2, er)
        assert same(call.results(), want2), rep
    del g
    print("capture ok", flush=True)


def concurrent():
    """the promise of include/pvw_hip.h for pvw_shamir_evaluate_wide_corrected / _erasures: two threads on one context overlap
    calls of different shapes, every result equals the serial one bit for bit, nothing is left in a workspace"""
    N = 140
    p = _params(N)
    rng = random.Random(58)
    jobs = []
    for k, (S, t, count, pm, T) in enumerate(((5, 4, 12, SECP_N, 9), (12, 20, 70, P255, 65), (7, 9, 50, P64, 30), (12, 3, 40, P17, 4))):
        idx, rows, _ = sharing(p, N, S, t, pm, count, rng, tag=k)
        plans = plans_for(S, count, count - t - 1, k, rng)
        bent = plant(rows, plans, rng)
        er = pack([e for e, _ in plans], count) if k % 3 else None
        targets = targets_for(idx, plans, N, T, rng)
        layout = ("secret_major", "party_major")[k % 2]
        jobs.append(lambda idx=idx, bent=bent, t=t, pm=pm, er=er, targets=targets, layout=layout:
                    buffer_evaluate(p, idx, bent, t, pm, er, targets, layout))
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


def repair():
    """one mid-size shape against planted truth (the cubic host form is not run here): 4 secrets, count 160, t 79 (r = 80) on a
    context with n = 200; 20 columns erased (junk) and 30 overwritten in every row (2 * 30 + 20 = 80 <= r); the targets are all 200
    indices, so every held, wrong, erased and never-dealt share comes back as dealt"""
    rng = random.Random(59)
    n, S, count, t, pm = 200, 4, 160, 79, SECP_N
    p = _params(n)
    s = torch.cuda.Stream(device=DEV)
    polys = [[rng.randrange(pm) for _ in range(t + 1)] for _ in range(S)]
    truth = [[sum(a * pow(i + 1, j, pm) for j, a in enumerate(poly)) % pm for i in range(n)] for poly in polys]
    idx = rng.sample(range(n), count)
    held = [[truth[srow][i] for i in idx] for srow in range(S)]
    plans = []
    for srow in range(S):
        cols = rng.sample(range(count), 50)
        plans.append((sorted(cols[:20]), sorted(cols[20:])))
        for c in cols[20:]:
            held[srow][c] = (held[srow][c] + 1 + rng.randrange(pm - 1)) % pm
        for c in cols[:20]:
            held[srow][c] = U64 if c % 2 else rng.getrandbits(256)
    rows = words([v for row in held for v in row], (S, count))
    er = pack([e for e, _ in plans], count)
    for layout in ("secret_major", "party_major"):
        val, out, nerr, col, mask = device_evaluate(p, idx, rows, t, pm, er, list(range(n)), layout, s)
        assert nerr.tolist() == [30] * S and ints(out) == [poly[0] for poly in polys], layout
        assert ints(val.reshape(S * n, 4)) == [v for row in truth for v in row], layout
        for srow, (_, errs) in enumerate(plans):
            assert [c for c in range(count) if (int(mask[srow][c // 64]) >> (c % 64)) & 1] == errs
    val = buffer_evaluate(p, idx, rows, t, pm, er, list(range(n)), "secret_major")[0]
    assert ints(val.reshape(S * n, 4)) == [v for row in truth for v in row]
    print("repair ok", flush=True)


def loop():
    """the whole chain on the device over the secp256k1 order at n = 9, t = 2 (r = 6), D = 4 dealers: deal
    (deal_party_shares_wide) -> c2 of two parties tampered in every dealer's limb-0 ciphertext by another scalar's encoding (a
    clean report, another value) and one party's share flagged (2^70 on one coefficient of one of its limb ciphertexts: a
    saturated noise) -> pvw_decrypt_all_checked_device, [party][dealer NL + w] -> pvw_shamir_wide_erasure_mask_device on that
    report in place -> the fold in place -> pvw_shamir_evaluate_wide_erasures_device in place, strides (1, D), every dealer a
    secret, targets 0 .. n.  2 * 2 + 1 <= r: the repaired parties' values equal the dealt shares (pvw_shamir_shares_wide), and the
    party that joins at index n gets the dealt polynomial's value there."""
    rng = random.Random(61)
    n, k, l, D, t, pm, lb = 9, 32, 8, 4, 2, SECP_N, 52
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    nl = P.shamir_wide_limbs(pm, lb)
    V = D * nl
    secrets = [pm - 1 - rng.randrange(1 << 100) for _ in range(D)]
    seeds = seeds_for(V, tag=12)
    cts = P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds, limb_bits=lb)
    cts = [ct for row in cts for ct in row]                          # vector d * NL + w
    dealt = [ints(row) for row in P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds[::nl], host=True)]   # dealer d draws under seeds[d NL]
    tampered = sorted(rng.sample(range(n), 2))
    flagged = rng.choice([i for i in range(n) if i not in tampered])
    quiet = p.encode_scalar(777, P.REPR_NTT).astype(object)
    e = np.zeros((p.L, p.l), dtype=np.uint64)
    e[:, 1] = [(1 << 70) % q for q in p.moduli()]
    loud = p.ntt_forward(e).astype(object) + quiet
    qq = np.array(p.moduli(), dtype=object)[:, None]
    for d in range(D):
        for party in tampered:
            ct = cts[d * nl]
            ct.c2[party] = ((ct.c2[party].astype(object) + quiet) % qq).astype(np.uint64)
        ct = cts[d * nl + d % nl]
        ct.c2[flagged] = ((ct.c2[flagged].astype(object) + loud) % qq).astype(np.uint64)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    pmw = api._wide_modulus(pm)
    d_sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
    c1, c2 = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2 for c in cts]))
    limbs = torch.zeros((n, V), dtype=torch.int64, device=DEV)
    noise = torch.zeros((n, V), dtype=torch.int64, device=DEV)
    status = torch.zeros((n, V), dtype=torch.int32, device=DEV)
    d_mask = torch.full((D, 1), 5, dtype=torch.int64, device=DEV)
    idx = np.arange(n, dtype=np.uint64)
    tg = np.arange(n + 1, dtype=np.uint64)
    val = torch.full((D, n + 1, 4), -1, dtype=torch.int64, device=DEV)
    out = torch.zeros((D, 4), dtype=torch.int64, device=DEV)
    nerr = torch.full((D,), 9, dtype=torch.int32, device=DEV)
    col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    emask = torch.full((D, 1), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    p._call("pvw_decrypt_all_checked_device", 0, n, ptr(d_sk), ptr(c1), ptr(c2), V, P.REPR_NTT, ptr(limbs), ptr(noise), ptr(status), sp)
    p._call("pvw_shamir_wide_erasure_mask_device", ptr(status), ptr(noise), P.DEC_LOSSY, p.noise_bound(), n, D, nl, V, nl, 1, ptr(d_mask), sp)
    folded = P.shamir_wide_from_limbs_device(p, limbs, pm, lb, layout="limb_minor", num_limbs=nl, stream=s)   # [n * D][4]
    p._call("pvw_shamir_evaluate_wide_erasures_device", nptr(pmw), t, nptr(idx), n, ptr(folded), D, 1, D, ptr(d_mask), nptr(tg), n + 1,
            ptr(val), ptr(out), ptr(nerr), ptr(col), ptr(emask), sp)
    s.synchronize()
    assert u64(d_mask).reshape(-1).tolist() == [1 << flagged] * D, "the checked decrypt flags exactly the loud share"
    assert ints(u64(out)) == [v % pm for v in secrets] and nerr.cpu().tolist() == [2] * D
    assert col.cpu().tolist() == [D if i in tampered else 0 for i in range(n)]
    assert u64(emask).reshape(-1).tolist() == [sum(1 << i for i in tampered)] * D
    got = [ints(row) for row in u64(val)]
    for d in range(D):
        assert got[d][:n] == dealt[d], ("held and repaired shares are the dealt ones", d)
        xs, ys, x, at = (1, 2, 3), dealt[d][:3], n + 1, 0            # degree 2: the value at the point n + 1 through three dealt shares
        for j in range(3):
            num = den = 1
            for i in range(3):
                if i != j:
                    num, den = num * (x - xs[i]) % pm, den * (xs[j] - xs[i]) % pm
            at = (at + ys[j] * num * pow(den, -1, pm)) % pm
        assert got[d][n] == at, ("the joining party", d)
    print("loop ok", flush=True)

CASES = {f.__name__: f for f in (null, far, groups, capture, concurrent, repair, loop)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("small"):
        small(int(sys.argv[1][5:]))
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_EVALUATE_OK")

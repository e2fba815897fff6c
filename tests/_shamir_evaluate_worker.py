"""Share repair on the device: the decode of 8.11 followed by shamir_ym_kernel, the public matrices of a target
group (shamir_target_scale_kernel, shamir_cauchy_kernel, shamir_powers_kernel, shamir_dpowers_kernel), three products by
shamir_matmul_kernel and shamir_evaluate_finish_kernel, against pvw_shamir_evaluate_corrected_host bit for bit on values, out,
nerr, col_err and err_mask; the host-buffer form (both copy paths, staged pieces, passes, target groups, hygiene); stream
capture; a full-size sharing against planted truth; the protocol loop closed; concurrent calls on one context.
torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_evaluate.py; prints
SHAMIR_EVALUATE_OK."""
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
from _shamir_correct_worker import (DEV, DISTINCT, INVALID_PARAMETERS, P17, _params, bend, bent_sharing, clean_rows, dev, host_corrected,  # noqa: E402
                                    laid_out, nptr, ptr, same, system, unreduced)
from test_shamir_host import secrets_for, seeds_for  # noqa: E402


def host_evaluated(idx, rows, t, pm, targets, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape
    ix, tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
    values = np.full((S, len(tg)), 3, np.uint64)
    out, nerr, col = np.full(S, 7, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32)
    mask = np.full((S, (count + 63) // 64), 5, np.uint64)
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_evaluate_corrected_host(pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(tg), len(tg), nptr(values), nptr(out),
                                                      nptr(nerr), nptr(col), nptr(mask)), lib)
    return values, out, nerr, col, mask


def host_tiled(idx, rows, t, pm, targets):
    """the host routine's report on rows whose row s repeats row s % DISTINCT: it decodes the distinct rows once (every output
    but col_err is per row, and col_err is the sum over the rows)"""
    S = rows.shape[0]
    if S <= DISTINCT:
        return host_evaluated(idx, rows, t, pm, targets)
    assert all(np.array_equal(rows[s], rows[s % DISTINCT]) for s in range(DISTINCT, S))
    values, out, nerr, _, mask = host_evaluated(idx, rows[:DISTINCT], t, pm, targets)
    pick = np.arange(S) % DISTINCT
    values, out, nerr, mask = values[pick], out[pick], nerr[pick], mask[pick]
    col = np.zeros(rows.shape[1], np.uint32)
    for c in range(rows.shape[1]):
        col[c] = int(((mask[:, c // 64] >> np.uint64(c % 64)) & np.uint64(1)).sum())
    return values, out, nerr, col, mask


class DeviceCall:
    """one pvw_shamir_evaluate_corrected_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, t, pm, targets, layout="secret_major"):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, pm
        self.S, self.count = rows.shape
        self.ix, self.tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.refill()

    def refill(self):
        self.values = torch.full((self.S, len(self.tg)), 3, dtype=torch.int64, device=DEV)
        self.out = torch.full((self.S,), -1, dtype=torch.int64, device=DEV)
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV)
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV)
        self.mask = torch.full((self.S, (self.count + 63) // 64), 5, dtype=torch.int64, device=DEV)

    def enqueue(self, stream_ptr, only_values=False):
        rest = (None, None, None, None) if only_values else (ptr(self.out), ptr(self.nerr), ptr(self.col), ptr(self.mask))
        return self.p._lib.pvw_shamir_evaluate_corrected_device(self.p._h, self.pm, self.t, nptr(self.ix), self.count, ptr(self.d_sh), self.S,
                                                                self.ss, self.ps, nptr(self.tg), len(self.tg), ptr(self.values), *rest,
                                                                stream_ptr)

    def results(self):
        return (self.values.cpu().numpy().view(np.uint64), self.out.cpu().numpy().view(np.uint64), self.nerr.cpu().numpy().view(np.uint32),
                self.col.cpu().numpy().view(np.uint32), self.mask.cpu().numpy().view(np.uint64))


def device_evaluated(p, idx, rows, t, pm, targets, layout, stream):
    call = DeviceCall(p, idx, rows, t, pm, targets, layout)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffers_evaluated(p, idx, rows, t, pm, targets, layout):
    arr, _ = laid_out(rows, layout)
    values, out, nerr, col, mask = P.shamir_evaluate_corrected(p, idx, arr.tolist(), t, pm, targets, layout=layout)
    return values, np.array(out, dtype=np.uint64), nerr, col, mask


def diff(got, want):
    return [np.argwhere(x != y)[:4].tolist() if x.shape == y.shape else "shape" for x, y in zip(got, want)]


def targets_for(idx, wrong, T, mode, N, rng):
    """T targets: 0 none of the points; 1 the columns in order (again from the first when T is larger); 2 the wrong columns, then
    the right ones; 3 a shuffled mix of columns and other indices with repeats"""
    count = len(idx)
    off = rng.sample(range(N, N + 4096), T)
    if mode == 0:
        return off
    if mode == 1:
        return [idx[j % count] for j in range(T)]
    if mode == 2:
        cols = sorted(wrong) + [c for c in range(count) if c not in wrong]
        return [idx[cols[j % count]] for j in range(T)]
    mix = [idx[rng.randrange(count)] if j % 2 else off[j] for j in range(T)]
    if T >= 3:
        mix[2] = mix[0]
    rng.shuffle(mix)
    return mix


def grid(nt):
    """device == host on all five outputs at t + 1 = nt and every r of the lane and chunk edges (E + 1 on both sides of 64 and 65;
    at t + 1 = 128 count = 255 .. 258 crosses the 4 waves x 64 terms of one chunk of the product), T and S rotating through
    their values, both layouts, unreduced words, the three primes and the four target mixes in turn.  Matrix A: the rows carry,
    in turn, no error, one, exactly E, another E disjoint from those, E + 1, and errors only inside columns 0..t.  Matrix B: one
    whole column overwritten, in rows that carry no other error, one, and E - 1 others."""
    N = 512
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(100 + nt), np.random.default_rng(100 + nt)
    reds = (127, 128, 129, 130) if nt == 128 else (0, 1, 2, 3, 126, 127, 128, 129, 130, 131)
    counts, widths, primes = (1, 3, 4, 5, 130), (1, 2, 63, 64, 65, 130), (P61, P62, P17)
    a = (1, 2, 5, 64, 65, 128).index(nt)
    for b, r in enumerate(reds):
        t, count, S, T, pm = nt - 1, nt + r, counts[(a + b) % 5], widths[(a + b) % 6], primes[(a + 2 * b) % 3]
        E = r // 2
        idx, secrets, rows = clean_rows(p, N, S, t, pm, count, rng, tag=a * 16 + b)
        cols = list(range(count))
        set_a = rng.sample(cols, E)
        rest = [c for c in cols if c not in set_a]
        plans = [[], rng.sample(cols, min(1, E)), set_a, rng.sample(rest, E), rng.sample(cols, min(E + 1, count)),
                 rng.sample(cols[:t + 1], min(E, t + 1))]
        A = rows.copy()
        for k in range(min(S, DISTINCT)):
            bend(A, k, plans[k], pm, rng)
        for k in range(DISTINCT, S):
            A[k] = A[k % DISTINCT]
        bad_col = rng.randrange(count)
        B = rows.copy()
        extra = [[], rng.sample([c for c in cols if c != bad_col], min(1, max(E - 1, 0))), rng.sample([c for c in cols if c != bad_col], max(E - 1, 0))]
        for k in range(min(S, DISTINCT)):
            bend(B, k, [bad_col] + extra[k % 3], pm, rng)
        for k in range(DISTINCT, S):
            B[k] = B[k % DISTINCT]
        wrong_a = set(c for k in range(min(S, DISTINCT)) for c in plans[k])
        wrong_b = set([bad_col] + [c for k in range(min(S, DISTINCT)) for c in extra[k % 3]])
        for name, mat, plan, wrong in (("A", A, plans, wrong_a), ("B", B, None, wrong_b)):
            words = unreduced(mat, pm, nrng)
            for k in range(DISTINCT, S):
                words[k] = words[k % DISTINCT]
            targets = targets_for(idx, wrong, T, (b + (name == "B")) % 4, N, rng)
            want = host_tiled(idx, words, t, pm, targets)
            if S <= DISTINCT:                            # one decode yields every report: the four are the corrected call's
                assert same(want[1:], host_corrected(idx, words, t, pm)), (nt, r)
            # what was planted is repaired: at every target that is a column, the dealt share (a false decode at these p: about
            # count^E / p; P17 is left out)
            if pm != P17:
                for k in range(S):
                    planted = plan[k % DISTINCT] if plan is not None else [bad_col] + extra[(k % DISTINCT) % 3]
                    if len(planted) <= E:
                        for j, tg in enumerate(targets):
                            if tg in idx:
                                assert want[0][k, j] == rows[k, idx.index(tg)], (nt, r, k, j)
                    elif r >= 1:
                        assert want[2][k] == UNDECODABLE and not want[0][k].any(), (nt, r, k)
            for layout in ("secret_major", "party_major"):
                got = device_evaluated(p, idx, words, t, pm, targets, layout, s)
                assert same(got, want), (name, nt, r, S, T, pm, layout, diff(got, want))
        print(f"grid t+1={nt} r={r} S={S} T={T} ok", flush=True)


def buffers():
    """the host-buffer form == the device form == the host routine (both copy paths: secret-major rows go up as they lie, by a
    2D copy, party-major ones packed); nothing that depends on the shares is left behind after a call, nor after a refused one;
    out, nerr, col_err and err_mask may be left out"""
    N = 200
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(13), np.random.default_rng(13)
    for S, t, count, T, pm in ((1, 0, 1, 1, P17), (5, 4, 5, 9, P61), (7, 9, 77, 100, P62), (30, 64, 150, 70, P61)):
        idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
        targets = targets_for(idx, set(), T, 3, N, rng)
        want = host_evaluated(idx, rows, t, pm, targets)
        for layout in ("secret_major", "party_major"):
            got = buffers_evaluated(p, idx, rows, t, pm, targets, layout)
            assert same(got, want), ("host-buffer", S, t, count, layout, diff(got, want))
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= 3 * S * count + 2 * S * T + S, ("residue", S, t, count, layout, nz, scanned)
            got = device_evaluated(p, idx, rows, t, pm, targets, layout, s)
            assert same(got, want), ("device", S, t, count, layout, diff(got, want))
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= 2 * S * count + S * T, ("residue", S, t, count, layout, nz, scanned)
    # a refused call stages nothing and leaves nothing: the residue report still reads clean
    ix, tg = np.array(idx, dtype=np.uint64), np.array(targets, dtype=np.uint64)
    arr, (ss, ps) = laid_out(rows, "secret_major")
    values = np.zeros((S, T), np.uint64)
    bad_tg = tg.copy()
    bad_tg[1] = pm - 1
    rc = p._lib.pvw_shamir_evaluate_corrected(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(bad_tg), T, nptr(values), None, None, None, None)
    assert rc == INVALID_PARAMETERS and "target" in _ffi.last_error(p._lib) and not values.any()
    assert api._secret_residue(p)[0] == 0
    # values alone
    api._check(p._lib.pvw_shamir_evaluate_corrected(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(tg), T, nptr(values), None, None, None,
                                                    None), p._lib)
    assert np.array_equal(values, want[0])
    call = DeviceCall(p, idx, rows, t, pm, targets)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(s.cuda_stream), only_values=True), p._lib)
    s.synchronize()
    assert np.array_equal(call.results()[0], want[0])
    assert api._secret_residue(p)[0] == 0
    print("buffers ok", flush=True)


def pieces():
    """several pieces (the tuning build).  PVW_STAGE_BYTES: the host-buffer form stages floor(budget / item) secrets at a time, item
    = (count + 1 + ceil(count / 64) + T) 8 + 4 bytes.  PVW_EVALUATE_GROUP_BYTES: the targets go in groups of floor(budget / per),
    per = (count + 2 (E + 1) + 2) 8 + 4 bytes a target, whole blocks of 64 above 64.  PVW_CORRECT_PIECE_BYTES: the kernels walk over
    floor(budget / per) secrets a pass, per = (2 count + r + E + 1 + 3 Tg + 2) 8 bytes.  Every combination equals the host routine
    in both layouts, col_err summed over the pieces."""
    _ffi.select("tuning")
    N, S, t, count, T, pm = 100, 23, 6, 40, 150, P61
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(14), np.random.default_rng(14)
    idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
    targets = targets_for(idx, set(), T, 3, N, rng)
    want = host_evaluated(idx, rows, t, pm, targets)
    assert (want[3] > 0).sum() >= 3 and (want[2] == UNDECODABLE).any() and (want[2] == (count - t - 1) // 2).any()
    r = count - t - 1
    E = r // 2

    def check(tag):
        for layout in ("secret_major", "party_major"):
            got = buffers_evaluated(p, idx, rows, t, pm, targets, layout)
            assert same(got, want), (tag, "host-buffer", layout, diff(got, want))
            assert api._secret_residue(p)[0] == 0
            got = device_evaluated(p, idx, rows, t, pm, targets, layout, s)
            assert same(got, want), (tag, "device", layout, diff(got, want))
            assert api._secret_residue(p)[0] == 0

    item = (count + 1 + 1 + T) * 8 + 4
    group = (count + 2 * (E + 1) + 2) * 8 + 4
    secret = lambda Tg: (2 * count + r + E + 1 + 3 * Tg + 2) * 8  # noqa: E731
    settings = [
        ("stage", {"PVW_STAGE_BYTES": 5 * item + 7}),                                  # 5 secrets a piece: 4 full pieces and one of 3
        ("groups64", {"PVW_EVALUATE_GROUP_BYTES": 70 * group}),                        # 70 -> 64 targets a group: 64, 64, 22
        ("groups7", {"PVW_EVALUATE_GROUP_BYTES": 7 * group + 5}),                      # 7 targets a group: 21 full groups and one of 3
        ("passes", {"PVW_CORRECT_PIECE_BYTES": 4 * secret(T) + 3}),                    # 4 secrets a pass: 5 full passes and one of 3
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
    """under stream capture in a fresh context, where nothing has sized the workspace, the call is refused with the error of the
    corrected call there and the capture survives empty; after one sizing call outside capture a captured call replays, and every
    replay reports on the shares that are in the buffer then: another error pattern each time, the same targets"""
    N, S, t, count, T, pm = 300, 9, 70, 200, 90, P61
    rng, nrng = random.Random(15), np.random.default_rng(15)
    p = _params(N)
    idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
    targets = targets_for(idx, set(), T, 3, N, rng)
    want = host_evaluated(idx, rows, t, pm, targets)
    call = DeviceCall(p, idx, rows, t, pm, targets)
    s0 = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg, (rc, msg)
    values, out, nerr, col, mask = call.results()                  # nothing was enqueued: the buffers keep their fill
    assert (values == 3).all() and (out == np.uint64(U64)).all() and (nerr == 9).all() and (col == 9).all() and (mask == 5).all()
    del g0
    # sized by one call outside capture, on the stream that is then captured
    s1 = torch.cuda.Stream(device=DEV)
    api._check(call.enqueue(C.c_void_p(s1.cuda_stream)), p._lib)
    s1.synchronize()
    assert same(call.results(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s1):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    api._check(rc, p._lib)
    E = (count - t - 1) // 2
    for rep in range(2):
        # new shares at the SAME points: the captured call carries the indices and targets it was made with
        full = P.shamir_shares(p, secrets_for(S, pm, rng), t, pm, seeds=seeds_for(S, tag=50 + rep), host=True)
        fresh = unreduced(full[:, idx], pm, nrng)
        bend(fresh, rep, rng.sample(range(count), E), pm, rng)
        bend(fresh, 5 + rep, rng.sample(range(count), 1 + rep), pm, rng)
        bend(fresh, 8 - rep, rng.sample(range(count), E + 1), pm, rng)
        call.d_sh.copy_(dev(fresh))
        call.values.fill_(3), call.out.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_evaluated(idx, fresh, t, pm, targets)
        assert want2[2][rep] == E and want2[2][5 + rep] == 1 + rep and want2[2][8 - rep] == UNDECODABLE
        got = call.results()
        assert same(got, want2), (rep, diff(got, want2))
        assert api._secret_residue(p)[0] == 0
    del g
    print("capture ok", flush=True)


def full():
    """against planted truth, not the host routine: pvw_shamir_shares_device makes S = 64 sharings of degree 2047 among n = 4160
    parties; the first 4096 are the input (r = 2048, E = 1024), 1024 of their columns are overwritten, and the targets are all 4160
    indices: values equals the untouched shares everywhere, the 64 parties that were never an input included.  One column more:
    every row is zero (a false decode: tests/_shamir_correct_worker.py, full)."""
    rng = random.Random(16)
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
    planted = rng.sample(range(2048), 300) + rng.sample(range(2048, count), 724)
    extra = next(c for c in range(count) if c not in planted)
    ix, tg = np.arange(count, dtype=np.uint64), np.arange(n, dtype=np.uint64)
    values = torch.full((S, n), 3, dtype=torch.int64, device=DEV)
    out = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    nerr = torch.full((S,), 9, dtype=torch.int32, device=DEV)
    run = lambda: p._call("pvw_shamir_evaluate_corrected_device", pm, t, nptr(ix), count, ptr(d_sh), S, n, 1, nptr(tg), n, ptr(values),  # noqa: E731
                          ptr(out), ptr(nerr), None, None, sp)
    junk = torch.from_numpy(np.random.default_rng(16).integers(1, pm, size=(S, len(planted)), dtype=np.int64)).to(DEV)
    with torch.cuda.stream(s):
        d_sh[:, planted] = (d_sh[:, planted] + junk) % pm
    run()
    s.synchronize()
    assert (nerr.cpu().numpy() == 1024).all()
    assert out.cpu().numpy().view(np.uint64).tolist() == [v % pm for v in secrets]
    assert torch.equal(values, truth), torch.nonzero(values != truth)[:4].tolist()
    with torch.cuda.stream(s):
        d_sh[:, extra] = (d_sh[:, extra] + 12345) % pm
    run()
    s.synchronize()
    assert (nerr.cpu().numpy().view(np.uint32) == UNDECODABLE).all() and not out.any().item() and not values.any().item()
    assert api._secret_residue(p)[0] == 0
    print("full ok", flush=True)


def loop():
    """the loop closed (n = 8, t = 2, D = 5, p = 2^61 - 1 > n + 1: r = 5, E = 2): deal -> what every party decrypts from every dealer
    mod p, [party][dealer], read in place -> two parties, party 0 among them, report junk for every dealer -> evaluated at those
    two parties' indices and at index n, a party that joins: the values are the dealt shares (for the new index: the dealers'
    polynomials through three honest parties' shares, in Python integers)"""
    rng = random.Random(17)
    n, k, l, t, D, pm = 8, 32, 8, 2, 5, P61
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    secrets = [pm - 1 - rng.randrange(1 << 20) for _ in range(D)]
    cts = P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds_for(D, tag=3))
    keys = [pt.secret_key for pt in parties]
    vals = np.asarray(P.decrypt_many_checked(cts, keys, 0, plain_modulus=pm).values).reshape(n, D).copy()
    dealt = vals.copy()
    tampered = (0, 5)
    for party in tampered:
        for d in range(D):
            vals[party, d] = (int(vals[party, d]) + 1 + rng.randrange(pm - 1)) % pm
    targets = list(tampered) + [n]
    values, out, nerr, col, mask = P.shamir_evaluate_corrected(p, list(range(n)), vals.tolist(), t, pm, targets, layout="party_major")
    assert out == secrets and nerr.tolist() == [2] * D and col.tolist() == [D * int(i in tampered) for i in range(n)]
    honest = [1, 2, 3]
    bx = [i + 1 for i in honest]
    w = _basis_weights(bx, pm)
    for d in range(D):
        assert [int(v) for v in values[d, :2]] == [int(dealt[i, d]) for i in tampered], d
        assert int(values[d, 2]) == _interpolate(bx, [int(dealt[i, d]) for i in honest], w, n + 1, pm), d
    assert api._secret_residue(p)[0] == 0
    print("loop ok", flush=True)


def concurrent():
    """the promise of include/pvw_hip.h for pvw_shamir_reconstruct_corrected and pvw_shamir_evaluate_corrected: threads on one
    context overlap both calls with different shapes, every result equals the serial one bit for bit, and no workspace that went
    from one call to the other keeps anything that depends on the shares"""
    N = 200
    p = _params(N)
    rng, nrng = random.Random(18), np.random.default_rng(18)
    jobs = []
    for k, (S, t, count, T, pm) in enumerate(((5, 4, 12, 9, P61), (30, 20, 90, 70, P62), (7, 9, 77, 0, P61), (12, 3, 40, 0, P17), (3, 30, 64, 130, P61),
                                              (64, 2, 9, 0, P62))):
        idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng, tag=k)
        layout = ("secret_major", "party_major")[k % 2]
        arr = laid_out(rows, layout)[0].tolist()
        if T:
            targets = targets_for(idx, set(), T, 3, N, rng)
            call = lambda idx=idx, arr=arr, t=t, pm=pm, targets=targets, layout=layout: buffers_tuple(  # noqa: E731
                P.shamir_evaluate_corrected(p, idx, arr, t, pm, targets, layout=layout))
        else:
            call = lambda idx=idx, arr=arr, t=t, pm=pm, layout=layout: buffers_tuple(  # noqa: E731
                P.shamir_reconstruct_corrected(p, idx, arr, t, pm, layout=layout))
        jobs.append(call)
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
                got = jobs[j]()
                if not same(got, serial[j]):
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


def buffers_tuple(res):
    return tuple(np.asarray(x, dtype=np.uint64) if isinstance(x, list) else x for x in res)


CASES = {f.__name__: f for f in (buffers, pieces, capture, full, loop, concurrent)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("grid"):
        grid(int(sys.argv[1][4:]))
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_EVALUATE_OK")

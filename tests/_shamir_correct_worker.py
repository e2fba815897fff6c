"""Corrected Shamir reconstruction on the device: shamir_matmul_kernel, shamir_bm_kernel and
shamir_correct_finish_kernel against pvw_shamir_reconstruct_corrected_host bit for bit on out, nerr, col_err and err_mask; the
checked call beside the corrected one; the host-buffer form (both copy paths, several staged pieces, hygiene); stream capture;
a full-size sharing against planted truth; the protocol loop closed with tampered parties.
torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_correct.py; prints
SHAMIR_CORRECT_OK."""
import ctypes as C
import os
import random
import sys

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import TEST_MODULI  # noqa: E402
from _shamir_correct_util import P61, P62, U64, UNDECODABLE  # noqa: E402
from test_shamir_host import secrets_for, seeds_for  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
P17 = 65537
INVALID_PARAMETERS = 1
DISTINCT = 6                                             # rows the host routine sees per matrix (it is cubic in count per row)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def nptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _params(n, k=2, l=8, moduli=TEST_MODULI):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()


def laid_out(rows, layout):
    """rows [S][count] (numpy) as the caller's matrix and its two strides"""
    S, count = rows.shape
    if layout == "secret_major":
        return np.ascontiguousarray(rows), (count, 1)
    return np.ascontiguousarray(rows.T), (1, S)


def host_corrected(idx, rows, t, pm, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape
    ix = np.array(idx, dtype=np.uint64)
    out, nerr, col = np.full(S, 7, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32)
    mask = np.full((S, (count + 63) // 64), 5, np.uint64)
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_reconstruct_corrected_host(pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(out), nptr(nerr), nptr(col),
                                                         nptr(mask)), lib)
    return out, nerr, col, mask


def host_tiled(idx, rows, t, pm):
    """the host routine's report on rows whose row s repeats row s % DISTINCT: it decodes the distinct rows once (every output
    but col_err is per row, and col_err is the sum over the rows)"""
    S = rows.shape[0]
    if S <= DISTINCT:
        return host_corrected(idx, rows, t, pm)
    assert all(np.array_equal(rows[s], rows[s % DISTINCT]) for s in range(DISTINCT, S))
    out, nerr, _, mask = host_corrected(idx, rows[:DISTINCT], t, pm)
    pick = np.arange(S) % DISTINCT
    out, nerr, mask = out[pick], nerr[pick], mask[pick]
    col = np.zeros(rows.shape[1], np.uint32)
    for c in range(rows.shape[1]):
        col[c] = int(((mask[:, c // 64] >> np.uint64(c % 64)) & np.uint64(1)).sum())
    return out, nerr, col, mask


class DeviceCall:
    """one pvw_shamir_reconstruct_corrected_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, t, pm, layout="secret_major"):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, pm
        self.S, self.count = rows.shape
        self.ix = np.array(idx, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.refill()

    def refill(self):
        self.out = torch.full((self.S,), -1, dtype=torch.int64, device=DEV)
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV)
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV)
        self.mask = torch.full((self.S, (self.count + 63) // 64), 5, dtype=torch.int64, device=DEV)

    def enqueue(self, stream_ptr):
        return self.p._lib.pvw_shamir_reconstruct_corrected_device(self.p._h, self.pm, self.t, nptr(self.ix), self.count, ptr(self.d_sh),
                                                                   self.S, self.ss, self.ps, ptr(self.out), ptr(self.nerr), ptr(self.col),
                                                                   ptr(self.mask), stream_ptr)

    def results(self):
        return (self.out.cpu().numpy().view(np.uint64), self.nerr.cpu().numpy().view(np.uint32), self.col.cpu().numpy().view(np.uint32),
                self.mask.cpu().numpy().view(np.uint64))


def device_corrected(p, idx, rows, t, pm, layout, stream):
    call = DeviceCall(p, idx, rows, t, pm, layout)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def unreduced(rows, pm, rng):
    """every other word as share + p (p < 2^62: it fits)"""
    mask = rng.integers(0, 2, size=rows.shape).astype(np.uint64)
    return rows + mask * np.uint64(pm)


def bend(rows, s, cols, pm, rng):
    """a nonzero amount added mod p to row s in every column of cols"""
    for c in cols:
        rows[s, c] = np.uint64((int(rows[s, c]) % pm + 1 + rng.randrange(pm - 1)) % pm)


def mask_of(cols, count):
    m = np.zeros((count + 63) // 64, np.uint64)
    for c in cols:
        m[c // 64] |= np.uint64(1 << (c % 64))
    return m


def clean_rows(p, N, S, t, pm, count, rng, tag):
    """S sharings of degree t (the first DISTINCT distinct, the rest repeating them) at `count` scattered parties of N"""
    D = min(S, DISTINCT)
    secrets = secrets_for(D, pm, rng)
    full = P.shamir_shares(p, secrets, t, pm, seeds=seeds_for(D, tag=tag), host=True)
    idx = rng.sample(range(N), count)
    pick = [s % D for s in range(S)]
    return idx, [secrets[s] % pm for s in pick], full[:, idx][pick]


def grid(nt):
    """device == host on all four outputs at t + 1 = nt and every r of the lane and chunk edges (E + 1 on both sides of 64 and
    65), S rotating through its values, both layouts, unreduced words, the three primes in turn.  Matrix A: the rows carry, in
    turn, no error, one, exactly E, another E disjoint from those, E + 1, and errors only inside columns 0..t.  Matrix B: one
    whole column overwritten, in rows that carry no other error, one, and E - 1 others."""
    N = 512
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(nt), np.random.default_rng(nt)
    reds, counts, primes = (0, 1, 2, 3, 126, 127, 128, 129, 130, 131), (1, 3, 4, 5, 130), (P61, P62, P17)
    a = (1, 2, 4, 5, 64, 65).index(nt)
    for b, r in enumerate(reds):
        t, count, S, pm = nt - 1, nt + r, counts[(a + b) % 5], primes[(a + 2 * b) % 3]
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
        for name, mat, plan in (("A", A, plans), ("B", B, None)):
            words = unreduced(mat, pm, nrng)
            for k in range(DISTINCT, S):
                words[k] = words[k % DISTINCT]
            want = host_tiled(idx, words, t, pm)
            # what was planted is what the host routine reports (a false decode at these p: about count^E / p; P17 is left out)
            if plan is not None and pm != P17:
                for k in range(S):
                    planted = plan[k % DISTINCT]
                    if len(planted) <= E:
                        assert want[0][k] == secrets[k] and want[1][k] == len(planted) and np.array_equal(want[3][k], mask_of(planted, count)), (nt, r, k)
                    elif r >= 1:
                        assert want[1][k] == UNDECODABLE and want[0][k] == 0 and not want[3][k].any(), (nt, r, k)
            if plan is None and E >= 1 and pm != P17:
                assert want[2][bad_col] == S and want[0].tolist() == secrets, (nt, r)
            for layout in ("secret_major", "party_major"):
                got = device_corrected(p, idx, words, t, pm, layout, s)
                assert same(got, want), (name, nt, r, S, pm, layout, [np.flatnonzero(x != y)[:4].tolist() if x.shape == y.shape else "shape" for x, y in zip(got, want)])
        print(f"grid t+1={nt} r={r} S={S} ok", flush=True)


def versus():
    """one bad share in column 0, a basis column of the checked call: pvw_shamir_reconstruct_checked_device returns a wrong out[s]
    and flags every extra of s; the corrected call returns the dealt secret and names the column"""
    N, S, t, count, pm = 64, 5, 3, 12, P61
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    rng = random.Random(11)
    idx, secrets, rows = clean_rows(p, N, S, t, pm, count, rng, tag=1)
    rows = rows.copy()
    bend(rows, 2, [0], pm, rng)
    ix, d_sh = np.array(idx, dtype=np.uint64), dev(rows)
    out = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    bad = torch.full((S,), 9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p._call("pvw_shamir_reconstruct_checked_device", pm, t, nptr(ix), count, ptr(d_sh), S, count, 1, ptr(out), ptr(bad), None, sp)
    s.synchronize()
    chk = out.cpu().numpy().view(np.uint64).tolist()
    assert chk[2] != secrets[2] and [v for k, v in enumerate(chk) if k != 2] == [v for k, v in enumerate(secrets) if k != 2]
    assert bad.cpu().numpy().tolist() == [0, 0, count - t - 1, 0, 0]
    got = device_corrected(p, idx, rows, t, pm, "secret_major", s)
    assert got[0].tolist() == secrets and got[1].tolist() == [0, 0, 1, 0, 0]
    assert got[2].tolist() == [1] + [0] * (count - 1) and got[3][:, 0].tolist() == [0, 0, 1, 0, 0]
    assert same(got, host_corrected(idx, rows, t, pm))
    print("versus ok", flush=True)


def bent_sharing(p, N, S, t, pm, count, rng, nrng, tag=0):
    """rows with different error sets (none, one, E, E + 1 in turn) and unreduced words"""
    idx, secrets, rows = clean_rows(p, N, min(S, DISTINCT), t, pm, count, rng, tag)
    E = (count - t - 1) // 2
    rows = rows[[k % rows.shape[0] for k in range(S)]].copy()
    for k in range(S):
        bend(rows, k, rng.sample(range(count), min((0, 1, E, E + 1)[k % 4], E + 1 if E else 0)), pm, rng)
    return idx, unreduced(rows, pm, nrng)


def buffers():
    """the host-buffer form == the device form == the host routine (both copy paths: secret-major rows go up as they lie, by a
    2D copy, party-major ones packed); no staged share, secret or locator value is left behind after a call, nor after a refused
    one; nerr, col_err and err_mask may be left out"""
    N = 200
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(3), np.random.default_rng(3)
    for S, t, count, pm in ((1, 0, 1, P17), (5, 4, 5, P61), (7, 9, 77, P62), (30, 64, 150, P61)):
        idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
        want = host_corrected(idx, rows, t, pm)
        for layout in ("secret_major", "party_major"):
            arr, _ = laid_out(rows, layout)
            out, nerr, col, mask = P.shamir_reconstruct_corrected(p, idx, arr.tolist(), t, pm, layout=layout)
            assert same((np.array(out, dtype=np.uint64), nerr, col, mask), want), ("host-buffer", S, t, count, layout)
            assert same(device_corrected(p, idx, rows, t, pm, layout, s), want), ("device", S, t, count, layout)
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= 2 * S * count + S, ("residue", S, t, count, layout, nz, scanned)
    # a refused call stages nothing and leaves nothing: the residue report still reads clean
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    arr, (ss, ps) = laid_out(rows, "secret_major")
    out = np.zeros(S, np.uint64)
    rc = p._lib.pvw_shamir_reconstruct_corrected(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(out), None, None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib)
    assert api._secret_residue(p)[0] == 0
    # out alone
    ix = np.array(idx, dtype=np.uint64)
    api._check(p._lib.pvw_shamir_reconstruct_corrected(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(out), None, None, None), p._lib)
    assert np.array_equal(out, want[0])
    call = DeviceCall(p, idx, rows, t, pm)
    torch.cuda.synchronize()
    api._check(p._lib.pvw_shamir_reconstruct_corrected_device(p._h, pm, t, nptr(call.ix), count, ptr(call.d_sh), S, ss, ps, ptr(call.out), None,
                                                              None, None, C.c_void_p(s.cuda_stream)), p._lib)
    s.synchronize()
    assert np.array_equal(call.results()[0], want[0])
    print("buffers ok", flush=True)


def pieces():
    """several pieces (the tuning build): the host-buffer form under a small PVW_STAGE_BYTES stages floor(budget / item) secrets
    at a time, item = (count + 1 + ceil(count / 64)) 8 + 4 bytes; the device form under a small PVW_CORRECT_PIECE_BYTES walks
    the kernels over 4 secrets at a time.  Both layouts equal the host routine, col_err summed over the pieces."""
    _ffi.select("tuning")
    N, S, t, count, pm = 100, 23, 6, 40, P61
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(4), np.random.default_rng(4)
    idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
    want = host_corrected(idx, rows, t, pm)
    assert (want[2] > 0).sum() >= 3 and (want[1] == UNDECODABLE).any() and (want[1] == (count - t - 1) // 2).any()
    item = (count + 1 + 1) * 8 + 4
    os.environ["PVW_STAGE_BYTES"] = str(5 * item + 7)                       # 5 secrets a piece: 4 full pieces and one of 3
    try:
        for layout in ("secret_major", "party_major"):
            arr, _ = laid_out(rows, layout)
            out, nerr, col, mask = P.shamir_reconstruct_corrected(p, idx, arr.tolist(), t, pm, layout=layout)
            assert same((np.array(out, dtype=np.uint64), nerr, col, mask), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_STAGE_BYTES", None)
    r = count - t - 1
    per = (count + r + r // 2 + 1) * 8 + 4
    os.environ["PVW_CORRECT_PIECE_BYTES"] = str(4 * per + 3)                # 4 secrets a pass: 5 full passes and one of 3
    try:
        for layout in ("secret_major", "party_major"):
            assert same(device_corrected(p, idx, rows, t, pm, layout, s), want), layout
        arr, _ = laid_out(rows, "party_major")
        out, nerr, col, mask = P.shamir_reconstruct_corrected(p, idx, arr.tolist(), t, pm, layout="party_major")
        assert same((np.array(out, dtype=np.uint64), nerr, col, mask), want)
        assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_CORRECT_PIECE_BYTES", None)
    print("pieces ok", flush=True)


def capture():
    """under stream capture in a fresh context, where nothing has sized the workspace, the call is refused with the error of the
    checked call there and the capture survives empty; after one sizing call outside capture a captured call replays, and every
    replay reports on the shares that are in the buffer then: another error pattern each time"""
    N, S, t, count, pm = 300, 9, 70, 200, P61
    rng, nrng = random.Random(5), np.random.default_rng(5)
    p = _params(N)
    idx, rows = bent_sharing(p, N, S, t, pm, count, rng, nrng)
    want = host_corrected(idx, rows, t, pm)
    call = DeviceCall(p, idx, rows, t, pm)
    s0 = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg, (rc, msg)
    out, nerr, col, mask = call.results()                          # nothing was enqueued: the buffers keep their fill
    assert (out == np.uint64(U64)).all() and (nerr == 9).all() and (col == 9).all() and (mask == 5).all()
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
        # new shares at the SAME points: the captured call carries the indices it was made with
        full = P.shamir_shares(p, secrets_for(S, pm, rng), t, pm, seeds=seeds_for(S, tag=40 + rep), host=True)
        fresh = unreduced(full[:, idx], pm, nrng)
        bend(fresh, rep, rng.sample(range(count), E), pm, rng)
        bend(fresh, 5 + rep, rng.sample(range(count), 1 + rep), pm, rng)
        bend(fresh, 8 - rep, rng.sample(range(count), E + 1), pm, rng)
        call.d_sh.copy_(dev(fresh))
        call.out.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_corrected(idx, fresh, t, pm)
        assert want2[1][rep] == E and want2[1][5 + rep] == 1 + rep and want2[1][8 - rep] == UNDECODABLE
        assert same(call.results(), want2), rep
        assert api._secret_residue(p)[0] == 0
    del g
    print("capture ok", flush=True)


def full():
    """against planted truth, not the host routine: pvw_shamir_shares_device makes S = 64 sharings of degree 2047 among n = 4096
    parties (r = 2048, E = 1024).  1024 whole columns overwritten, 300 of them among the first 2048: the secrets come back,
    nerr = 1024 everywhere, the mask is the planted set and col_err = 64 exactly there.  One column more: every secret is
    undecodable -- a row with 1025 errors lies within 1024 of another polynomial with probability below C(4096, 1024)^2 / p^(t+1)
    by a union bound over the pairs of error sets, which at p = 2^61 - 1 and t + 1 = 2048 is far below 2^-100000."""
    rng = random.Random(6)
    n, S, t, pm = 4096, 64, 2047, P61
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
    planted = rng.sample(range(2048), 300) + rng.sample(range(2048, n), 724)
    extra = next(c for c in range(n) if c not in planted)
    ix = np.arange(n, dtype=np.uint64)
    out = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    nerr = torch.full((S,), 9, dtype=torch.int32, device=DEV)
    col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    mask = torch.full((S, n // 64), 5, dtype=torch.int64, device=DEV)
    run = lambda: p._call("pvw_shamir_reconstruct_corrected_device", pm, t, nptr(ix), n, ptr(d_sh), S, n, 1, ptr(out), ptr(nerr), ptr(col),  # noqa: E731
                          ptr(mask), sp)
    # junk differs from the share it replaces in every place (a 61-bit word added mod p, never 0)
    junk = torch.from_numpy(np.random.default_rng(6).integers(1, pm, size=(S, len(planted)), dtype=np.int64)).to(DEV)
    with torch.cuda.stream(s):
        d_sh[:, planted] = (d_sh[:, planted] + junk) % pm
    run()
    s.synchronize()
    assert out.cpu().numpy().view(np.uint64).tolist() == [v % pm for v in secrets]
    assert (nerr.cpu().numpy() == 1024).all()
    want_mask = np.tile(mask_of(planted, n), (S, 1))
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), want_mask)
    want_col = np.zeros(n, np.int32)
    want_col[planted] = S
    assert np.array_equal(col.cpu().numpy(), want_col)
    with torch.cuda.stream(s):
        d_sh[:, extra] = (d_sh[:, extra] + 12345) % pm
    run()
    s.synchronize()
    assert (nerr.cpu().numpy().view(np.uint32) == UNDECODABLE).all() and not out.any().item() and not mask.any().item() and not col.any().item()
    print("full ok", flush=True)


def system(n, k, l, moduli):
    p = _params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


def loop():
    """the loop closed with bad parties (n = 8, t = 2, D = 5, p = 2^61 - 1: r = 5, E = 2): deal -> what every party decrypts from
    every dealer mod p, [party][dealer] -> two parties, party 0 among them, report junk for every dealer -> every dealer's secret
    comes back and col_err names exactly those two parties, each with all D dealers"""
    rng = random.Random(7)
    n, k, l, t, D, pm = 8, 32, 8, 2, 5, P61
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    secrets = [pm - 1 - rng.randrange(1 << 20) for _ in range(D)]
    cts = P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds_for(D, tag=3))
    keys = [pt.secret_key for pt in parties]
    vals = np.asarray(P.decrypt_many_checked(cts, keys, 0, plain_modulus=pm).values).reshape(n, D).copy()
    out, nerr, col, mask = P.shamir_reconstruct_corrected(p, list(range(n)), vals.tolist(), t, pm, layout="party_major")
    assert out == secrets and not nerr.any() and not col.any() and not mask.any()
    for party in (0, 5):
        for d in range(D):
            vals[party, d] = (int(vals[party, d]) + 1 + rng.randrange(pm - 1)) % pm
    out, nerr, col, mask = P.shamir_reconstruct_corrected(p, list(range(n)), vals.tolist(), t, pm, layout="party_major")
    assert out == secrets and nerr.tolist() == [2] * D
    assert col.tolist() == [D * int(i in (0, 5)) for i in range(n)] and mask[:, 0].tolist() == [(1 << 0) | (1 << 5)] * D
    # the checked call on the same matrix takes party 0 into its basis: every secret wrong
    chk, bad, _ = P.shamir_reconstruct_checked(p, list(range(n)), vals.tolist(), t, pm, layout="party_major")
    assert all(a != b for a, b in zip(chk, secrets)) and bad.tolist() == [n - t - 1] * D
    print("loop ok", flush=True)


CASES = {f.__name__: f for f in (versus, buffers, pieces, capture, full, loop)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("grid"):
        grid(int(sys.argv[1][4:]))
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_CORRECT_OK")

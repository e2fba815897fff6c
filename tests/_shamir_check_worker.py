"""Checked Shamir reconstruction on the device: shamir_weights_kernel + shamir_interp_kernel against
pvw_shamir_reconstruct_checked_host bit for bit on out, bad and col_bad, the host-buffer form (several staged pieces, hygiene),
stream capture, a full-size sharing made by pvw_shamir_shares_device, more secrets than one launch holds, and the protocol loop
closed with every party checked.
torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_check.py; prints
SHAMIR_CHECK_OK."""
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
from test_shamir_check_host import P61, P62, restated  # noqa: E402
from test_shamir_host import secrets_for, seeds_for  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
P17 = 65537
U64 = (1 << 64) - 1
INVALID_PARAMETERS = 1


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


def host_checked(idx, rows, t, pm, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape
    ix = np.array(idx, dtype=np.uint64)
    out, bad, col = np.zeros(S, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32)
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_reconstruct_checked_host(pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(out), nptr(bad), nptr(col)), lib)
    return out, bad, col


class DeviceCall:
    """one pvw_shamir_reconstruct_checked_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, t, pm, layout):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, pm
        self.S, self.count = rows.shape
        self.ix = np.array(idx, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.out = torch.full((self.S,), -1, dtype=torch.int64, device=DEV)
        self.bad = torch.full((self.S,), 9, dtype=torch.int32, device=DEV)
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV)

    def enqueue(self, stream_ptr):
        return self.p._lib.pvw_shamir_reconstruct_checked_device(self.p._h, self.pm, self.t, nptr(self.ix), self.count, ptr(self.d_sh), self.S,
                                                                 self.ss, self.ps, ptr(self.out), ptr(self.bad), ptr(self.col), stream_ptr)

    def results(self):
        return (self.out.cpu().numpy().view(np.uint64), self.bad.cpu().numpy().view(np.uint32), self.col.cpu().numpy().view(np.uint32))


def device_checked(p, idx, rows, t, pm, layout, stream):
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


def grid():
    """device == host on every (t + 1, T) of the frame's edges, S rotating through its values (every S meets every T and every
    t + 1), both layouts, unreduced words, the three primes in turn; a clean sharing first (the host routine must give the
    secrets back with nothing flagged), then one bent extra, one bent basis share and one bent column"""
    N = 512
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(1), np.random.default_rng(1)
    terms, targets, counts = (1, 2, 4, 5, 64, 65, 257, 301), (1, 2, 64, 65, 130), (1, 3, 4, 5, 130)
    primes = (P61, P62, P17)
    for a, nt in enumerate(terms):
        for b, T in enumerate(targets):
            t, count, S, pm = nt - 1, nt - 1 + T, counts[(a + b) % 5], primes[(a + 2 * b) % 3]
            secrets, seeds = secrets_for(S, pm, rng), seeds_for(S, tag=a * 8 + b)
            full = P.shamir_shares(p, secrets, t, pm, seeds=seeds, host=True)
            idx = rng.sample(range(N), count)                      # unsorted, non-contiguous
            rows = unreduced(full[:, idx], pm, nrng)
            want = host_checked(idx, rows, t, pm)
            assert want[0].tolist() == [v % pm for v in secrets] and not want[1].any() and not want[2].any(), ("clean", nt, T, S)
            for layout in ("secret_major", "party_major"):
                assert same(device_checked(p, idx, rows, t, pm, layout, s), want), ("clean", nt, T, S, pm, layout)
            bent = rows.copy()
            if T > 1:
                bent[S // 2, t + 1 + (T - 2) // 2] ^= np.uint64(1)            # one extra
            if S > 1:
                bent[S - 1, t // 2] += np.uint64(3)                        # one basis share of another secret
            if T > 2:
                bent[:, count - 1] = nrng.integers(0, pm, size=S, dtype=np.uint64)   # one whole column
            want = host_checked(idx, bent, t, pm)
            if S > 1 and T > 1:
                assert want[1][S - 1] == T - 1 and want[0][S - 1] != secrets[S - 1] % pm
            assert same(host_checked(idx, bent, t, pm, "party_major"), want)
            for layout in ("secret_major", "party_major"):
                assert same(device_checked(p, idx, bent, t, pm, layout, s), want), ("bent", nt, T, S, pm, layout)
        print(f"grid t+1={nt} ok", flush=True)


def far():
    """a far-apart index set (one index near 2^40, one just below p - 1, none contiguous), shares by pow and % in Python:
    device == host == the restatement, at each prime"""
    p = _params(8)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(2)
    t, count, S = 5, 70, 5
    for pm in (P61, P62, P17):
        top = pm - 1
        idx = {top - 1, min((1 << 40) - 3, top - 7), 0}
        while len(idx) < count:
            idx.add(rng.randrange(top))
        idx = list(idx)
        rng.shuffle(idx)
        polys = [[rng.randrange(pm) for _ in range(t + 1)] for _ in range(S)]
        rows = [[sum(a[j] * pow(i + 1, j, pm) for j in range(t + 1)) % pm for i in idx] for a in polys]
        rows[1][t + 3] = (rows[1][t + 3] + 1) % pm
        rows[4][2] = (rows[4][2] + 5) % pm
        out, bad, col = restated(idx, rows, t, pm)
        want = (np.array(out, dtype=np.uint64), np.array(bad, dtype=np.uint32), np.array(col, dtype=np.uint32))
        arr = np.array(rows, dtype=np.uint64)
        assert same(host_checked(idx, arr, t, pm), want), pm
        for layout in ("secret_major", "party_major"):
            assert same(device_checked(p, idx, arr, t, pm, layout, s), want), (pm, layout)
    print("far ok", flush=True)


def sharing(p, N, S, t, pm, count, rng, nrng, tag=0):
    secrets, seeds = secrets_for(S, pm, rng), seeds_for(S, tag=tag)
    full = P.shamir_shares(p, secrets, t, pm, seeds=seeds, host=True)
    idx = rng.sample(range(N), count)
    rows = unreduced(full[:, idx], pm, nrng)
    rows[S // 3, t + 2] ^= np.uint64(8)
    rows[S - 1, 1] += np.uint64(1)
    return idx, rows


def buffers():
    """the host-buffer form == the device form == the host routine (both layouts: rows uploaded as they lie, and packed); no
    staged share or secret is left behind after a call, nor after a refused one; bad and col_bad may be left out"""
    N = 200
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng, nrng = random.Random(3), np.random.default_rng(3)
    for S, t, count, pm in ((1, 0, 1, P17), (5, 4, 5, P61), (7, 9, 77, P62), (130, 64, 199, P61)):
        idx, rows = sharing(p, N, S, t, pm, count, rng, nrng) if count > t + 2 else (rng.sample(range(N), count), nrng.integers(0, pm, size=(S, count), dtype=np.uint64))
        want = host_checked(idx, rows, t, pm)
        for layout in ("secret_major", "party_major"):
            arr, _ = laid_out(rows, layout)
            out, bad, col = P.shamir_reconstruct_checked(p, idx, arr.tolist(), t, pm, layout=layout)
            assert same((np.array(out, dtype=np.uint64), bad, col), want), ("host-buffer", S, t, count, layout)
            assert same(device_checked(p, idx, rows, t, pm, layout, s), want), ("device", S, t, count, layout)
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= S * count + S, ("residue", S, t, count, layout, nz, scanned)
    # a refused call stages nothing and leaves nothing: the residue report still reads clean
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    arr, (ss, ps) = laid_out(rows, "secret_major")
    out = np.zeros(S, np.uint64)
    rc = p._lib.pvw_shamir_reconstruct_checked(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(out), None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib)
    assert api._secret_residue(p)[0] == 0
    # out alone
    ix = np.array(idx, dtype=np.uint64)
    api._check(p._lib.pvw_shamir_reconstruct_checked(p._h, pm, t, nptr(ix), count, nptr(arr), S, ss, ps, nptr(out), None, None), p._lib)
    assert np.array_equal(out, want[0])
    call = DeviceCall(p, idx, rows, t, pm, "secret_major")
    torch.cuda.synchronize()
    api._check(p._lib.pvw_shamir_reconstruct_checked_device(p._h, pm, t, nptr(call.ix), count, ptr(call.d_sh), S, ss, ps, ptr(call.out), None, None,
                                                            C.c_void_p(s.cuda_stream)), p._lib)
    s.synchronize()
    assert np.array_equal(call.results()[0], want[0])
    print("buffers ok", flush=True)


def pieces():
    """the host-buffer form through several staged pieces (the tuning build with a small PVW_STAGE_BYTES): a piece holds
    floor(budget / ((count + 1) 8 + 4)) secrets; both layouts equal the host routine, col_bad summed over the pieces"""
    _ffi.select("tuning")
    N, S, t, count, pm = 100, 23, 6, 40, P61
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    rng, nrng = random.Random(4), np.random.default_rng(4)
    idx, rows = sharing(p, N, S, t, pm, count, rng, nrng)
    rows[:, count - 2] = nrng.integers(0, pm, size=S, dtype=np.uint64)      # a bent column: every piece adds to col_bad
    want = host_checked(idx, rows, t, pm)
    assert want[2][count - 2] == S
    budget = 5 * ((count + 1) * 8 + 4) + 7                                  # 5 secrets a piece: 4 full pieces and one of 3
    os.environ["PVW_STAGE_BYTES"] = str(budget)
    try:
        assert budget // ((count + 1) * 8 + 4) == 5
        for layout in ("secret_major", "party_major"):
            arr, _ = laid_out(rows, layout)
            out, bad, col = P.shamir_reconstruct_checked(p, idx, arr.tolist(), t, pm, layout=layout)
            assert same((np.array(out, dtype=np.uint64), bad, col), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_STAGE_BYTES", None)
    print("pieces ok", flush=True)


def capture():
    """under stream capture in a fresh context, where nothing has sized the workspace, the call is refused with the error of
    multi-dealer encrypt and the capture survives empty; after one call with the same (degree, count) outside capture a captured
    call replays, and every replay reports on the shares that are in the buffer then"""
    N, S, t, count, pm = 300, 9, 70, 200, P61
    rng, nrng = random.Random(5), np.random.default_rng(5)
    p = _params(N)
    idx, rows = sharing(p, N, S, t, pm, count, rng, nrng)
    want = host_checked(idx, rows, t, pm)
    call = DeviceCall(p, idx, rows, t, pm, "secret_major")
    s0 = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg, (rc, msg)
    out, bad, col = call.results()                                 # nothing was enqueued: the buffers keep their fill
    assert (out == np.uint64(U64)).all() and (bad == 9).all() and (col == 9).all()
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
    for rep in range(2):
        # new shares at the SAME points: the captured call carries the indices it was made with
        full = P.shamir_shares(p, secrets_for(S, pm, rng), t, pm, seeds=seeds_for(S, tag=40 + rep), host=True)
        fresh = unreduced(full[:, idx], pm, nrng)
        fresh[rep, t + 1 + rep] ^= np.uint64(2)
        call.d_sh.copy_(dev(fresh))
        call.out.fill_(-1), call.bad.fill_(9), call.col.fill_(9)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_checked(idx, fresh, t, pm)
        assert want2[1][rep] == 1 and want2[2][t + 1 + rep] == 1
        assert same(call.results(), want2), rep
    del g
    print("capture ok", flush=True)


def full():
    """independent of the restatements: pvw_shamir_shares_device makes S = 64 sharings of degree 2047 among n = 4096 parties; all
    4096 columns in their natural order, strides (n, 1): out == the secrets, nothing flagged; then one flipped word in an extra
    column is flagged at exactly that (s, c)"""
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
    ix = np.arange(n, dtype=np.uint64)
    out = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    bad = torch.full((S,), 9, dtype=torch.int32, device=DEV)
    col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    run = lambda: p._call("pvw_shamir_reconstruct_checked_device", pm, t, nptr(ix), n, ptr(d_sh), S, n, 1, ptr(out), ptr(bad), ptr(col), sp)  # noqa: E731
    run()
    s.synchronize()
    assert out.cpu().numpy().view(np.uint64).tolist() == [v % pm for v in secrets]
    assert not bad.any().item() and not col.any().item()
    with torch.cuda.stream(s):
        d_sh[37, 3001] ^= 1 << 17
    run()
    s.synchronize()
    assert out.cpu().numpy().view(np.uint64).tolist() == [v % pm for v in secrets]
    b, c = bad.cpu().numpy(), col.cpu().numpy()
    assert b.sum() == 1 and b[37] == 1 and c.sum() == 1 and c[3001] == 1
    print("full ok", flush=True)


def system(n, k, l, moduli):
    p = _params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


def loop():
    """the loop closed with every party checked (n = 8, t = 2, D = 5, p = 2^61 - 1): deal -> aggregate -> every party's sum mod p
    -> the checked sum of the secrets over all n parties, nothing flagged; a tampered sum flags its party's column.  The dealer
    check: what every party decrypts from every dealer, [P][D] read party-major, gives every dealer's secret back with nothing
    flagged; a dealt matrix with one off-polynomial entry flags exactly that dealer"""
    rng = random.Random(7)
    n, k, l, t, D, pm = 8, 32, 8, 2, 5, P61
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    secrets = [pm - 1 - rng.randrange(1 << 20) for _ in range(D)]
    seeds = seeds_for(D, tag=3)
    cts = P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds)
    agg = P.aggregate_ciphertexts(cts)
    sums = [int(v) for v in P.decrypt_all_party_sums([agg], parties, plain_modulus=pm).values]
    idx = [5, 0, 7, 2, 1, 6, 3, 4]                                 # all n parties, the basis 5, 0, 7
    out, bad, col = P.shamir_reconstruct_checked(p, idx, [[sums[i] for i in idx]], t, pm)
    assert out == [sum(secrets) % pm] and not bad.any() and not col.any()
    bent = list(sums)
    bent[6] = (bent[6] + 1) % pm
    out, bad, col = P.shamir_reconstruct_checked(p, idx, [[bent[i] for i in idx]], t, pm)
    assert out == [sum(secrets) % pm] and bad.tolist() == [1] and col.tolist() == [int(i == 6) for i in idx]
    # the dealer check, D = 5 dealers: [P][D], party-major
    keys = [pt.secret_key for pt in parties]
    vals = np.asarray(P.decrypt_many_checked(cts, keys, 0, plain_modulus=pm).values).reshape(n, D)
    out, bad, col = P.shamir_reconstruct_checked(p, list(range(n)), vals.tolist(), t, pm, layout="party_major")
    assert out == [v % pm for v in secrets] and not bad.any() and not col.any()
    # n dealers through encrypt_all_party_shares / decrypt_all_party_shares_checked, one entry off its polynomial
    secrets = [rng.randrange(pm) for _ in range(n)]
    sh = P.shamir_shares(p, secrets, t, pm, seeds=seeds_for(n, tag=4), host=True)
    sh[3, 6] = (int(sh[3, 6]) + 12345) % pm
    cts = P.encrypt_all_party_shares(sh.tolist(), gpk, SEED)
    r = P.decrypt_all_party_shares_checked(cts, parties)
    vals = np.asarray(r.values).reshape(n, n)
    assert np.array_equal(vals, sh.T)
    out, bad, col = P.shamir_reconstruct_checked(p, list(range(n)), vals.tolist(), t, pm, layout="party_major")
    assert out == secrets and bad.tolist() == [int(d == 3) for d in range(n)] and col.tolist() == [int(i == 6) for i in range(n)]
    print("loop ok", flush=True)


def launches():
    """more secrets than one launch of shamir_interp_kernel holds (the grid's y dimension: 65535 groups of 4): S = 65535 * 4 + 5,
    so the second launch has one full group and one partial one.  count = 3, degree = 1: random rows on lines, column 2 bent in
    the first secret, on both sides of the launch boundary and in the last secret; both layouts == the host routine on out, bad
    and col_bad"""
    S, t, pm, idx = 65535 * 4 + 5, 1, P61, (0, 1, 2)
    p = _params(8)
    s = torch.cuda.Stream(device=DEV)
    nrng = np.random.default_rng(8)
    a = nrng.integers(0, pm, size=(2, S), dtype=np.uint64)
    rows = np.stack([(a[0] + a[1] * np.uint64(i + 1)) % np.uint64(pm) for i in idx], axis=1)   # a0 + 3 a1 < 2^63
    bent = (0, 262139, 262140, 262144)
    for b in bent:
        rows[b, 2] ^= np.uint64(1)
    want = host_checked(idx, rows, t, pm)
    assert np.array_equal(want[0], a[0]) and np.flatnonzero(want[1]).tolist() == list(bent) and want[2].tolist() == [0, 0, len(bent)]
    for layout in ("secret_major", "party_major"):
        assert laid_out(rows, layout)[1] == ((3, 1) if layout == "secret_major" else (1, S))
        assert same(device_checked(p, idx, rows, t, pm, layout, s), want), layout
    print("launches ok", flush=True)


CASES = {f.__name__: f for f in (grid, far, buffers, pieces, capture, full, launches, loop)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_CHECK_OK")

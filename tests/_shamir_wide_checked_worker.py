"""The receiving end over a prime field of up to 256 bits on the device: the general product against Python's
integers; shamir_wide_fold_kernel against pvw_shamir_wide_from_limbs_host; the weights and the product kernel against
pvw_shamir_reconstruct_wide_checked_host bit for bit on out, bad and col_bad (device-pointer and host-buffer forms); stream
capture; the chain deal -> decrypt_all -> fold -> checked reconstruction with every buffer in place; staging in several pieces;
key hygiene.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_wide_checked.py; prints SHAMIR_WIDE_CHECKED_OK."""
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
from test_shamir_wide_host import BLS_R, PRIMES, SECP_N, W256, ints, seeds_for  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
U64 = (1 << 64) - 1
P17, P64, P255 = 65537, 2**64 + 13, 2**255 - 19
INVALID_PARAMETERS = 1
SG, TC, WAVES = 4, 8, 4            # the product kernel's secrets per lane, terms per wave and chunk, waves


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def nptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def _params(n, k=2, l=8, moduli=TEST_MODULI):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()


def words(values, shape):
    return api._wide(values).reshape(*shape, 4)


def laid_out(rows, layout):
    """rows [S][count][4] (numpy) as the caller's matrix and its two strides, in elements"""
    S, count = rows.shape[:2]
    if layout == "secret_major":
        return np.ascontiguousarray(rows), (count, 1)
    return np.ascontiguousarray(rows.transpose(1, 0, 2)), (1, S)


def host_checked(idx, rows, t, pm, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape[:2]
    ix = np.array(idx, dtype=np.uint64)
    out, bad, col = np.zeros((S, 4), np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32)
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_reconstruct_wide_checked_host(nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(arr), S, ss, ps,
                                                            nptr(out), nptr(bad), nptr(col)), lib)
    return out, bad, col


class DeviceCall:
    """one pvw_shamir_reconstruct_wide_checked_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, t, pm, layout, bad=True, col=True):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, api._wide_modulus(pm)
        self.S, self.count = rows.shape[:2]
        self.ix = np.array(idx, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.out = torch.full((self.S, 4), -1, dtype=torch.int64, device=DEV)
        self.bad = torch.full((self.S,), 9, dtype=torch.int32, device=DEV) if bad else None
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV) if col else None

    def enqueue(self, stream_ptr):
        return self.p._lib.pvw_shamir_reconstruct_wide_checked_device(self.p._h, nptr(self.pm), self.t, nptr(self.ix), self.count,
                                                                      ptr(self.d_sh), self.S, self.ss, self.ps, ptr(self.out), ptr(self.bad),
                                                                      ptr(self.col), stream_ptr)

    def results(self):
        return (u64(self.out), None if self.bad is None else self.bad.cpu().numpy().view(np.uint32),
                None if self.col is None else self.col.cpu().numpy().view(np.uint32))


def device_checked(p, idx, rows, t, pm, layout, stream, **kw):
    call = DeviceCall(p, idx, rows, t, pm, layout, **kw)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffer_checked(p, idx, rows, t, pm, layout):
    arr, _ = laid_out(rows, layout)
    out, bad, col = P.shamir_reconstruct_wide_checked(p, idx, arr, t, pm, layout=layout)
    return api._wide(out), bad, col


def same(a, b):
    return all(x is None or np.array_equal(x, y) for x, y in zip(a, b))


def sharing(p, N, S, t, pm, count, rng, tag=0):
    """S sharings of degree t dealt on the host, the columns of `count` random parties picked out, every word that has room
    for it raised by a multiple of p: (idx, rows [S][count][4], secrets)"""
    secrets = [rng.getrandbits(256) for _ in range(S)]
    full = P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds_for(S, tag=tag), host=True)
    idx = rng.sample(range(N), count)
    vals = [[v + pm * ((W256 - v) // pm) if (s + c) % 2 else v for c, v in enumerate(row)] for s, row in enumerate(ints(full[:, idx]))]
    return idx, words([v for row in vals for v in row], (S, count)), [v % pm for v in secrets]


def bend(rows, s, c, rng):
    rows[s, c, rng.randrange(4)] ^= np.uint64(1 << rng.randrange(64))


def mul():
    """pvw_selftest_shamir_wide_mul == a b mod p on 0, 1, p - 1 and random operands in every combination, at three primes"""
    rng = random.Random(1)
    lib = _ffi.lib()
    p = _params(3)
    for pm in (PRIMES[0], P64, SECP_N):
        edge = [0, 1, pm - 1, rng.randrange(pm)]
        cases = [(a, b) for a in edge for b in edge] + [(rng.randrange(pm), rng.randrange(pm)) for _ in range(700)]
        a, b = api._wide([c[0] for c in cases]), api._wide([c[1] for c in cases])
        out = np.zeros((len(cases), 4), dtype=np.uint64)
        api._check(lib.pvw_selftest_shamir_wide_mul(p._h, nptr(api._wide_modulus(pm)), nptr(a), nptr(b), len(cases), nptr(out)), lib)
        assert ints(out) == [x * y % pm for x, y in cases], pm
    print("mul ok", flush=True)


def fold():
    """pvw_shamir_wide_from_limbs_device == pvw_shamir_wide_from_limbs_host: count 1, 70, 300 (beyond one workgroup), NL 1, 5,
    16, limb bits 16, 52, 62, both stride pairs, words up to 2^64 - 1"""
    nrng = np.random.default_rng(2)
    p = _params(3)
    s = torch.cuda.Stream(device=DEV)
    for count in (1, 70, 300):
        for nl, lb, pm in ((1, 16, P17), (1, 62, 2**61 - 1), (5, 52, SECP_N), (5, 62, P255), (16, 16, BLS_R), (16, 62, P64), (2, 52, 2**89 - 1)):
            planes = nrng.integers(0, 1 << 64, size=(nl, count), dtype=np.uint64)
            planes[0, 0], planes[nl - 1, count - 1] = np.uint64(U64), np.uint64(U64)
            want = api._wide(P.shamir_wide_from_limbs(planes.tolist(), pm, lb))
            got = P.shamir_wide_from_limbs_device(p, dev(planes), pm, lb, stream=s)
            s.synchronize()
            assert np.array_equal(u64(got), want), ("planes", count, nl, lb)
            side = dev(np.ascontiguousarray(planes.T))               # [count][NL]: strides (1, NL)
            got = P.shamir_wide_from_limbs_device(p, side, pm, lb, layout="limb_minor", stream=s)
            s.synchronize()
            assert np.array_equal(u64(got), want), ("side by side", count, nl, lb)
    print("fold ok", flush=True)


def checked():
    """device == host on out, bad and col_bad: count 1..3, 65, 70, 130 (one target, both sides of the 64-target block), degrees
    0, 1, count - 1 and those either side of the four-wave split (t + 1 = 3, 4, 5), of one chunk of 8 terms per wave (t + 1 = 32,
    33) and of two (64, 65); num_secrets 1, 3, 4, 5, 9 in turn; both layouts; a clean sharing with unreduced words, then deviations
    in the first, a middle and the last extra column and in a basis column; the device-pointer and the host-buffer form; NULL
    bad / col_bad; four primes in turn"""
    N = 140
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(3)
    primes, sizes = (P17, P64, P255, SECP_N), (1, 3, 4, 5, 9)
    k = 0
    for count in (1, 2, 3, 65, 70, 130):
        for t in sorted({0, 1, count - 1} | {d for d in (2, 3, 4, 31, 32, 63, 64, 66) if d < count}):
            if t >= count:
                continue
            S, pm = sizes[k % 5], primes[k % 4]
            k += 1
            T = count - t
            idx, rows, secrets = sharing(p, N, S, t, pm, count, rng, tag=k)
            want = host_checked(idx, rows, t, pm)
            assert ints(want[0]) == secrets and not want[1].any() and not want[2].any(), ("clean", count, t, S)
            for layout in ("secret_major", "party_major"):
                assert same(device_checked(p, idx, rows, t, pm, layout, s), want), ("clean", count, t, S, pm, layout)
            bent = rows.copy()
            if T > 1:
                for c in {t + 1, t + 1 + (T - 2) // 2, count - 1}:
                    bend(bent, rng.randrange(S), c, rng)
            if S > 1:
                bend(bent, S - 1, t // 2, rng)                     # a basis share
            want = host_checked(idx, bent, t, pm)
            if S > 1 and T > 1:
                assert want[1][S - 1] == T - 1 and ints(want[0])[S - 1] != secrets[S - 1]
            assert same(host_checked(idx, bent, t, pm, "party_major"), want)
            for layout in ("secret_major", "party_major"):
                assert same(device_checked(p, idx, bent, t, pm, layout, s), want), ("bent", count, t, S, pm, layout)
            if k % 3 == 0 or count == 130:
                layout = ("secret_major", "party_major")[k % 2]
                assert same(buffer_checked(p, idx, bent, t, pm, layout), want), ("host-buffer", count, t, S, pm, layout)
            if k % 4 == 0:
                assert same(device_checked(p, idx, bent, t, pm, "secret_major", s, bad=False), want), ("no bad", count, t)
                assert same(device_checked(p, idx, bent, t, pm, "party_major", s, col=False), want), ("no col_bad", count, t)
                assert same(device_checked(p, idx, bent, t, pm, "secret_major", s, bad=False, col=False), want), ("out alone", count, t)
        print(f"checked count={count} ok", flush=True)
    # words that mean 0 and 2^256 - 1 mod p: p itself and 2^256 - 1, degree 0
    for pm in primes:
        r = W256 % pm
        rows = words([0, pm, 0, pm, 0, W256, r, W256, r, W256], (2, 5))
        want = host_checked([4, 0, 9, 2, 7], rows, 0, pm)
        assert ints(want[0]) == [0, r] and not want[1].any() and not want[2].any()
        assert same(device_checked(p, [4, 0, 9, 2, 7], rows, 0, pm, "secret_major", s), want), pm
    # an index of 2^64 - 1: the point 2^64
    idx = [U64, 5, 0, U64 - 1, 77]
    polys = [[rng.randrange(P64) for _ in range(3)] for _ in range(3)]
    rows = words([sum(a[j] * pow(i + 1, j, P64) for j in range(3)) % P64 for a in polys for i in idx], (3, 5))
    want = host_checked(idx, rows, 2, P64)
    assert ints(want[0]) == [a[0] for a in polys] and not want[1].any()
    assert same(device_checked(p, idx, rows, 2, P64, "secret_major", s), want)
    print("checked ok", flush=True)


def capture():
    """under stream capture in a fresh context, where nothing has sized the workspace, the call is refused and the capture
    survives empty; after one call with the same (degree, count) outside capture a captured call replays, and every replay
    reports on the shares that are in the buffer then, with counters that start from 0"""
    N, S, t, count, pm = 140, 9, 40, 110, SECP_N
    rng = random.Random(5)
    p = _params(N)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    bend(rows, 2, t + 3, rng)
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
        full = P.shamir_shares_wide(p, [rng.getrandbits(256) for _ in range(S)], t, pm, seeds=seeds_for(S, tag=40 + rep), host=True)
        fresh = np.ascontiguousarray(full[:, idx])
        bend(fresh, rep, t + 1 + rep, rng)
        bend(fresh, 5 + rep, count - 1 - rep, rng)
        call.d_sh.copy_(dev(fresh))
        call.out.fill_(-1), call.bad.fill_(9), call.col.fill_(9)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_checked(idx, fresh, t, pm)
        assert want2[1].sum() == 2 and want2[1][rep] == 1 and want2[2][t + 1 + rep] == 1
        assert same(call.results(), want2), rep
    del g
    print("capture ok", flush=True)


def system(n, k, l, moduli):
    p = _params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


def loop():
    """five dealers over the secp256k1 order at n = 5, t = 2, nothing leaving the device between the steps: deal
    (pvw_deal_shares_wide_device) -> every party decrypts every limb of every dealer (pvw_decrypt_all_device, [party][dealer NL +
    w]) -> the fold in place, strides (1, NL), to [party][dealer][4] -> checked reconstruction in place, strides (1, D), every
    dealer a secret: the dealers' secrets, nothing flagged.  With one ciphertext's c2 row of party 4 replaced before the
    decrypt, col_bad names party 4 and bad the dealer"""
    rng = random.Random(7)
    n, k, l, D, t, pm, lb = 5, 32, 8, 5, 2, SECP_N, 52
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    nl = P.shamir_wide_limbs(pm, lb)
    V = D * nl
    secrets = [pm - 1 - rng.randrange(1 << 100) for _ in range(D)]
    pmw = api._wide_modulus(pm)
    s = torch.cuda.Stream(device=DEV)
    sp = C.c_void_p(s.cuda_stream)
    d_se = dev(api._wide(secrets))
    seeds = np.frombuffer(b"".join(seeds_for(V, tag=9)), dtype=np.uint8).copy()
    c1 = torch.zeros((V, k, p.L, l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((V, n, p.L, l), dtype=torch.int64, device=DEV)
    d_sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
    limbs = torch.zeros((n, V), dtype=torch.int64, device=DEV)
    idx = np.arange(n, dtype=np.uint64)
    out = torch.zeros((D, 4), dtype=torch.int64, device=DEV)
    bad = torch.full((D,), 9, dtype=torch.int32, device=DEV)
    col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p._call("pvw_deal_shares_wide_device", ptr(d_se), D, t, nptr(pmw), lb, nptr(seeds), ptr(c1), ptr(c2), P.REPR_NTT, sp)
    for tampered in (False, True):
        if tampered:
            with torch.cuda.stream(s):
                c2[1 * nl + 2, 4] = c2[1 * nl + 3, 4].clone()      # dealer 1, limb 2, party 4
        p._call("pvw_decrypt_all_device", 0, n, ptr(d_sk), ptr(c1), ptr(c2), V, P.REPR_NTT, ptr(limbs), sp)
        folded = P.shamir_wide_from_limbs_device(p, limbs, pm, lb, layout="limb_minor", num_limbs=nl, stream=s)   # [n * D][4]
        p._call("pvw_shamir_reconstruct_wide_checked_device", nptr(pmw), t, nptr(idx), n, ptr(folded), D, 1, D, ptr(out), ptr(bad), ptr(col), sp)
        s.synchronize()
        assert ints(u64(out)) == secrets, tampered
        if not tampered:
            assert not bad.any().item() and not col.any().item()
            sh = P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds_for(V, tag=9)[::nl], host=True)            # [D][n][4]
            assert np.array_equal(u64(folded).reshape(n, D, 4), sh.transpose(1, 0, 2))
        else:
            assert bad.cpu().tolist() == [0, 1, 0, 0, 0] and col.cpu().tolist() == [0, 0, 0, 0, 1]
    print("loop ok", flush=True)


def pieces():
    """the host-buffer form through several staged pieces (the tuning build with a small PVW_STAGE_BYTES): a piece holds
    floor(budget / ((count + 1) 32 + 4)) secrets; both layouts equal the host routine, col_bad summed over the pieces"""
    _ffi.select("tuning")
    os.environ.pop("PVW_STAGE_BYTES", None)
    N, S, t, count, pm = 100, 23, 6, 40, SECP_N
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    rng = random.Random(4)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    for srow in range(S):
        bend(rows, srow, count - 2, rng)                           # a bent column: every piece adds to col_bad
    bend(rows, 7, 3, rng)
    want = host_checked(idx, rows, t, pm)
    assert want[2][count - 2] == S
    budget = 5 * ((count + 1) * 32 + 4) + 7                        # 5 secrets a piece: 4 full pieces and one of 3
    os.environ["PVW_STAGE_BYTES"] = str(budget)
    try:
        for layout in ("secret_major", "party_major"):
            assert same(buffer_checked(p, idx, rows, t, pm, layout), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_STAGE_BYTES", None)
    print("pieces ok", flush=True)


def hygiene():
    """no staged share or secret is left behind after a host-buffer call (both layouts), nor after a refused one; the scanned
    regions are not empty"""
    N = 140
    p = _params(N)
    rng = random.Random(6)
    for S, t, count, pm in ((1, 0, 1, P17), (5, 4, 5, P64), (9, 9, 77, SECP_N)):
        idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
        want = host_checked(idx, rows, t, pm)
        for layout in ("secret_major", "party_major"):
            assert same(buffer_checked(p, idx, rows, t, pm, layout), want), (S, t, count, layout)
            nz, scanned = api._secret_residue(p)
            assert nz == 0 and scanned >= (S * count + S) * 4, ("residue", S, t, count, layout, nz, scanned)
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    out = np.zeros((S, 4), np.uint64)
    rc = p._lib.pvw_shamir_reconstruct_wide_checked(p._h, nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(rows), S, count, 1, nptr(out),
                                                    None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib) and not out.any()
    assert api._secret_residue(p)[0] == 0
    print("hygiene ok", flush=True)


CASES = {f.__name__: f for f in (mul, fold, checked, capture, loop, pieces, hygiene)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_CHECKED_OK")

"""Corrected reconstruction over a prime field of up to 256 bits on the device: the public matrices, the two
products, the wide Berlekamp-Massey kernel and the finish pass against pvw_shamir_reconstruct_wide_corrected_host bit for bit on
out, nerr, col_err and err_mask (device-pointer and host-buffer forms); the dynamic-LDS opt-in path against planted truth;
pieces and passes; hygiene; stream capture; the chain deal -> decrypt_all -> fold -> corrected reconstruction in place.  torch is
imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_wide_corrected.py;
prints SHAMIR_WIDE_CORRECTED_OK."""
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
from test_shamir_wide_host import SECP_N, W256, ints, seeds_for  # noqa: E402
from _shamir_wide_checked_worker import (DEV, INVALID_PARAMETERS, P17, P64, P255, U64, _params, bend, dev, laid_out, nptr, ptr,  # noqa: E402
                                         same, sharing, system, u64, words)

UNDECODABLE = P.SHAMIR_UNDECODABLE
PRIMES4 = (P17, P64, P255, SECP_N)


def host_corrected(idx, rows, t, pm, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape[:2]
    ix = np.array(idx, dtype=np.uint64)
    W = (count + 63) // 64
    out, nerr, col, mask = (np.full((S, 4), 9, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32),
                            np.full((S, W), 9, np.uint64))
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_reconstruct_wide_corrected_host(nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(arr), S, ss, ps,
                                                              nptr(out), nptr(nerr), nptr(col), nptr(mask)), lib)
    return out, nerr, col, mask


class DeviceCall:
    """one pvw_shamir_reconstruct_wide_corrected_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, t, pm, layout="secret_major", nerr=True, col=True, mask=True):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, api._wide_modulus(pm)
        self.S, self.count = rows.shape[:2]
        self.ix = np.array(idx, dtype=np.uint64)
        self.d_sh = dev(arr)
        W = (self.count + 63) // 64
        self.out = torch.full((self.S, 4), -1, dtype=torch.int64, device=DEV)
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV) if nerr else None
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV) if col else None
        self.mask = torch.full((self.S, W), -1, dtype=torch.int64, device=DEV) if mask else None

    def enqueue(self, stream_ptr):
        return self.p._lib.pvw_shamir_reconstruct_wide_corrected_device(self.p._h, nptr(self.pm), self.t, nptr(self.ix), self.count,
                                                                        ptr(self.d_sh), self.S, self.ss, self.ps, ptr(self.out),
                                                                        ptr(self.nerr), ptr(self.col), ptr(self.mask), stream_ptr)

    def results(self):
        return (u64(self.out), None if self.nerr is None else self.nerr.cpu().numpy().view(np.uint32),
                None if self.col is None else self.col.cpu().numpy().view(np.uint32), None if self.mask is None else u64(self.mask))


def device_corrected(p, idx, rows, t, pm, layout, stream, **kw):
    call = DeviceCall(p, idx, rows, t, pm, layout, **kw)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffer_corrected(p, idx, rows, t, pm, layout):
    arr, _ = laid_out(rows, layout)
    out, nerr, col, mask = P.shamir_reconstruct_wide_corrected(p, idx, arr, t, pm, layout=layout)
    return api._wide(out), nerr, col, mask


def spoil(rows, plan, rng):
    """a copy of rows with one bit flipped in the columns plan[s] of row s: the word read mod p changes by a power of two"""
    bent = rows.copy()
    for s, cols in enumerate(plan):
        for c in cols:
            bend(bent, s, c, rng)
    return bent


def error_plan(S, count, E, k, rng):
    """row s: 0, 1, E, E + 1 or E // 2 wrong columns in turn, each row its own set; row 0's set holds column 0 when it is not empty"""
    plan = []
    for s in range(S):
        nbad = min((0, 1, E, E + 1, E // 2)[(s + k) % 5], count)
        cols = rng.sample(range(count), nbad)
        if s == 0 and cols and 0 not in cols:
            cols[0] = 0
        plan.append(sorted(cols))
    return plan


def small(tp1):
    """device == host on all four outputs at t + 1 = tp1 and r in {0, 1, 2, 3, 8, 9, 126 .. 130} (count <= 140): both sides of the
    64-target block of either product, of the four-wave term split, of the 8-term chunk and of the 64-coefficient block of the
    locator; num_secrets 1, 3, 4, 5, 9 in turn; both layouts; unreduced words; rows with 0, 1, E, E + 1 and E / 2 errors, each
    its own set; NULL outputs; four primes in turn; the host-buffer form; the checked wide call beside it on a bad share in
    column 0"""
    N = 140
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(100 + tp1)
    sizes = (1, 3, 4, 5, 9)
    t = tp1 - 1
    k = tp1
    for r in (0, 1, 2, 3, 8, 9, 126, 127, 128, 129, 130):
        count, E = tp1 + r, r // 2
        if count > 140:
            continue
        S, pm = sizes[k % 5], PRIMES4[k % 4]
        k += 1
        idx, rows, secrets = sharing(p, N, S, t, pm, count, rng, tag=k)
        plan = error_plan(S, count, E, k, rng)
        bent = spoil(rows, plan, rng)
        want = host_corrected(idx, bent, t, pm)
        for srow, cols in enumerate(plan):                        # what the contract fixes about the planted rows
            if len(cols) <= E:
                assert ints(want[0])[srow] == secrets[srow] and want[1][srow] == len(cols), ("planted", tp1, r, srow)
                assert [c for c in range(count) if (int(want[3][srow][c // 64]) >> (c % 64)) & 1] == cols
            elif r and pm > 2**64:
                assert want[1][srow] == UNDECODABLE and not want[3][srow].any() and not want[0][srow].any(), ("beyond E", tp1, r, srow)
        for layout in ("secret_major", "party_major"):
            got = device_corrected(p, idx, bent, t, pm, layout, s)
            assert same(got, want), ("device", tp1, r, S, pm, layout, got[1], want[1])
        if k % 2 == 0 or r == 130:
            layout = ("secret_major", "party_major")[(k // 2) % 2]
            assert same(buffer_corrected(p, idx, bent, t, pm, layout), want), ("host-buffer", tp1, r, S, pm, layout)
        if k % 3 == 0:
            assert same(device_corrected(p, idx, bent, t, pm, "secret_major", s, nerr=False), want), ("no nerr", tp1, r)
            assert same(device_corrected(p, idx, bent, t, pm, "party_major", s, col=False, mask=False), want), ("no col_err, mask", tp1, r)
            assert same(device_corrected(p, idx, bent, t, pm, "secret_major", s, nerr=False, col=False, mask=False), want), ("out alone", tp1, r)
        if E >= 1 and plan[0] and len(plan[0]) <= E and t + 1 < count:
            # the checked call on the same shares: column 0 is in its basis, so it gets secret 0 wrong; the corrected call does not
            out = torch.zeros((S, 4), dtype=torch.int64, device=DEV)
            p._call("pvw_shamir_reconstruct_wide_checked_device", nptr(api._wide_modulus(pm)), t, nptr(np.array(idx, dtype=np.uint64)), count,
                    ptr(dev(bent)), S, count, 1, ptr(out), None, None, C.c_void_p(s.cuda_stream))
            s.synchronize()
            assert ints(u64(out))[0] != secrets[0] and ints(want[0])[0] == secrets[0], ("checked beside corrected", tp1, r)
        print(f"small t+1={tp1} r={r} S={S} ok", flush=True)
    if tp1 == 1:
        # words that mean 0 and 2^256 - 1 mod p: p itself and 2^256 - 1, degree 0, one of five wrong
        for pm in PRIMES4:
            rr = W256 % pm
            rows = words([0, pm, 0, pm, 1, W256, rr, W256, rr, 5], (2, 5))
            want = host_corrected([4, 0, 9, 2, 7], rows, 0, pm)
            assert ints(want[0]) == [0, rr] and want[1].tolist() == [1, 1] and want[2].tolist() == [0, 0, 0, 0, 2]
            assert same(device_corrected(p, [4, 0, 9, 2, 7], rows, 0, pm, "secret_major", s), want), pm
        # an index of 2^64 - 1: the point 2^64
        idx = [U64, 5, 0, U64 - 1, 77, 9, 31]
        polys = [[rng.randrange(P64) for _ in range(3)] for _ in range(3)]
        rows = words([sum(a[j] * pow(i + 1, j, P64) for j in range(3)) % P64 for a in polys for i in idx], (3, 7))
        bend(rows, 1, 0, rng)
        bend(rows, 2, 6, rng)
        bend(rows, 2, 3, rng)
        want = host_corrected(idx, rows, 2, P64)
        assert ints(want[0]) == [a[0] for a in polys] and want[1].tolist() == [0, 1, 2]
        assert same(device_corrected(p, idx, rows, 2, P64, "secret_major", s), want)
    print(f"small {tp1} ok", flush=True)


def lds():
    """The dynamic-LDS opt-in path against planted truth (the cubic host form cannot run at this size): count 2052, t 1, r 2050,
    E 1025 -- the two polynomials of one wave take 2 * 1026 * 32 = 65 664 bytes, above the 64 KiB a launch gets without asking
    -- over the secp256k1 order, S = 3.  A consistent row and a row with 1025 planted errors come back exactly.  A row with
    1026 planted errors of uniformly random nonzero value is undecodable: with E + 1 planted errors (the set B) on F, a second
    polynomial G within E of the row has D = G - F != 0 of degree <= t.  Outside B the row minus G is -D, nonzero except at D's
    at most t roots, and there are count - (E + 1) = t + E columns outside B (r = 2 E is even): at least E of them are off G, so
    G is within E only if D has t roots among them AND the errors equal D on ALL of B.  For each of the at most C(count, t) root
    sets and p - 1 scalings that happens with probability (p - 1)^-(E + 1): in all at most C(count, t) / p = 2052 / p < 2^-240.
    F itself is off in E + 1 columns."""
    count, t, pm, S = 2052, 1, SECP_N, 3
    E = (count - t - 1) // 2
    assert E == 1025 and 2 * (E + 1) * 32 == 65664 > 65536
    rng = random.Random(8)
    p = _params(7)
    s = torch.cuda.Stream(device=DEV)
    idx = rng.sample(range(1 << 40), count)
    polys = [[rng.randrange(pm) for _ in range(t + 1)] for _ in range(S)]
    vals = [[(a[0] + a[1] * (i + 1)) % pm for i in idx] for a in polys]
    bad1 = sorted(rng.sample(range(count), E))
    bad2 = sorted(rng.sample(range(count), E + 1))
    for c in bad1:
        vals[1][c] = (vals[1][c] + 1 + rng.randrange(pm - 1)) % pm
    for c in bad2:
        vals[2][c] = (vals[2][c] + 1 + rng.randrange(pm - 1)) % pm
    rows = words([v for row in vals for v in row], (S, count))
    out, nerr, col, mask = device_corrected(p, idx, rows, t, pm, "secret_major", s)
    assert ints(out) == [polys[0][0], polys[1][0], 0], "secrets"
    assert nerr.tolist() == [0, E, UNDECODABLE], nerr
    want_col = np.zeros(count, np.uint32)
    want_col[bad1] = 1
    assert np.array_equal(col, want_col)
    want_mask = np.zeros((S, (count + 63) // 64), np.uint64)
    for c in bad1:
        want_mask[1, c // 64] |= np.uint64(1 << (c % 64))
    assert np.array_equal(mask, want_mask)
    print("lds ok", flush=True)


def pieces():
    """the host-buffer form through both copy paths (dense rows by a 2D copy, party-major by a host repack) in several staged
    pieces, and the device form in several passes (the tuning build with a small PVW_STAGE_BYTES / PVW_CORRECT_PIECE_BYTES): all
    equal the host routine, col_err summed over the pieces; nothing secret is left behind after success nor after a refusal"""
    _ffi.select("tuning")
    for name in ("PVW_STAGE_BYTES", "PVW_CORRECT_PIECE_BYTES"):
        os.environ.pop(name, None)
    N, S, t, count, pm = 100, 23, 6, 40, SECP_N
    r = count - t - 1
    E = r // 2
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(4)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plan = error_plan(S, count, E, 0, rng)
    for cols in plan:
        if len(cols) < E and count - 2 not in cols:
            cols.append(count - 2)                                  # a bent column: every piece adds to col_err
    bent = spoil(rows, plan, rng)
    want = host_corrected(idx, bent, t, pm)
    assert want[2][count - 2] >= 10 and (want[1] == UNDECODABLE).any() and (want[1] == E).any()
    for layout in ("secret_major", "party_major"):                 # one piece, one pass
        assert same(buffer_corrected(p, idx, bent, t, pm, layout), want), layout
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= (S * count + S + S * count) * 4, ("residue", layout, nz, scanned)
    item = (count + 1) * 32 + 8 + 4
    os.environ["PVW_STAGE_BYTES"] = str(5 * item + 7)               # 5 secrets a piece: 4 full pieces and one of 3
    try:
        for layout in ("secret_major", "party_major"):
            assert same(buffer_corrected(p, idx, bent, t, pm, layout), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_STAGE_BYTES", None)
    per = (count + r + E + 1) * 32 + 4
    os.environ["PVW_CORRECT_PIECE_BYTES"] = str(4 * per + 3)        # 4 secrets a pass: 5 full passes and one of 3
    try:
        for layout in ("secret_major", "party_major"):
            assert same(device_corrected(p, idx, bent, t, pm, layout, s), want), layout
            assert same(buffer_corrected(p, idx, bent, t, pm, layout), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_CORRECT_PIECE_BYTES", None)
    # a refused call leaves nothing behind and writes nothing
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    out = np.zeros((S, 4), np.uint64)
    rc = p._lib.pvw_shamir_reconstruct_wide_corrected(p._h, nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(bent), S, count, 1, nptr(out),
                                                      None, None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib) and not out.any()
    assert api._secret_residue(p)[0] == 0
    print("pieces ok", flush=True)


def capture():
    """under stream capture in a fresh context, where nothing has sized the workspace, the call is refused with the error of the
    checked wide call there and the capture survives empty; after one sizing call outside capture a captured call replays, and
    every replay reports on the shares that are in the buffer then: new shares with another error pattern each time"""
    N, S, t, count, pm = 140, 9, 40, 110, SECP_N
    E = (count - t - 1) // 2
    rng = random.Random(5)
    p = _params(N)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    bent = spoil(rows, error_plan(S, count, E, 1, rng), rng)
    want = host_corrected(idx, bent, t, pm)
    call = DeviceCall(p, idx, bent, t, pm)
    s0 = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg, (rc, msg)
    out, nerr, col, mask = call.results()                          # nothing was enqueued: the buffers keep their fill
    assert (out == np.uint64(U64)).all() and (nerr == 9).all() and (col == 9).all() and (mask == np.uint64(U64)).all()
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
        fresh = spoil(np.ascontiguousarray(full[:, idx]), error_plan(S, count, E, 2 + rep, rng), rng)
        call.d_sh.copy_(dev(fresh))
        call.out.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_corrected(idx, fresh, t, pm)
        assert (want2[1] == UNDECODABLE).any() and (want2[1] == E).any() and not np.array_equal(want2[3], want[3])
        assert same(call.results(), want2), rep
    del g
    print("capture ok", flush=True)


def loop():
    """five dealers over the secp256k1 order at n = 5, t = 1, nothing leaving the device between the steps: deal
    (pvw_deal_shares_wide_device) -> every party decrypts every limb of every dealer (pvw_decrypt_all_device) -> the fold in
    place, strides (1, NL) -> corrected reconstruction in place, strides (1, D), every dealer a secret.  With party 0's
    ciphertext rows tampered before the decrypt (r = 3: one wrong share per secret is corrected) the secrets still come back
    and col_err and the mask name party 0, while the checked call on the same buffer, whose basis holds party 0, gets them
    wrong"""
    rng = random.Random(7)
    n, k, l, D, t, pm, lb = 5, 32, 8, 5, 1, SECP_N, 52
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
    nerr = torch.full((D,), 9, dtype=torch.int32, device=DEV)
    col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    mask = torch.full((D, 1), -1, dtype=torch.int64, device=DEV)
    cout = torch.zeros((D, 4), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    p._call("pvw_deal_shares_wide_device", ptr(d_se), D, t, nptr(pmw), lb, nptr(seeds), ptr(c1), ptr(c2), P.REPR_NTT, sp)
    for tampered in (False, True):
        if tampered:
            with torch.cuda.stream(s):
                for d in range(D):                                 # every dealer's limb 1 for party 0 replaced by its limb 2
                    c2[d * nl + 1, 0] = c2[d * nl + 2, 0].clone()
        p._call("pvw_decrypt_all_device", 0, n, ptr(d_sk), ptr(c1), ptr(c2), V, P.REPR_NTT, ptr(limbs), sp)
        folded = P.shamir_wide_from_limbs_device(p, limbs, pm, lb, layout="limb_minor", num_limbs=nl, stream=s)   # [n * D][4]
        p._call("pvw_shamir_reconstruct_wide_corrected_device", nptr(pmw), t, nptr(idx), n, ptr(folded), D, 1, D, ptr(out), ptr(nerr),
                ptr(col), ptr(mask), sp)
        p._call("pvw_shamir_reconstruct_wide_checked_device", nptr(pmw), t, nptr(idx), n, ptr(folded), D, 1, D, ptr(cout), None, None, sp)
        s.synchronize()
        assert ints(u64(out)) == secrets, tampered
        if not tampered:
            assert not nerr.any().item() and not col.any().item() and not mask.any().item()
            assert ints(u64(cout)) == secrets
        else:
            assert nerr.cpu().tolist() == [1] * D and col.cpu().tolist() == [D, 0, 0, 0, 0] and mask.cpu().tolist() == [[1]] * D
            assert all(a != b for a, b in zip(ints(u64(cout)), secrets)), "the checked call trusts party 0"
    print("loop ok", flush=True)


CASES = {f.__name__: f for f in (lds, pieces, capture, loop)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("small"):
        small(int(sys.argv[1][5:]))
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_CORRECTED_OK")

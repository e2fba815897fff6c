"""Reconstruction with erasures over a prime field of up to 256 bits on the device: the masked syndromes, the
erasure-locator / Forney / Berlekamp-Massey kernel, the locator values and the finish pass against
pvw_shamir_reconstruct_wide_erasures_host bit for bit on out, nerr, col_err and err_mask (device-pointer and host-buffer forms); a
NULL mask against the wide corrected device call; far rows over a small prime; the mask kernel against the host builder; the
dynamic-LDS opt-in path at both edges against planted truth; pieces and passes; hygiene; stream capture with another mask per
replay; concurrent calls; the chain deal -> checked decrypt-all -> mask -> fold -> reconstruction in place.  torch is imported
FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_wide_erasures.py; prints
SHAMIR_WIDE_ERASURES_OK."""
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
from _shamir_wide_checked_worker import (DEV, INVALID_PARAMETERS, P17, P64, P255, U64, _params, bend, dev, laid_out, nptr, ptr,  # noqa: E402
                                         same, sharing, system, u64, words)
from _shamir_wide_corrected_worker import DeviceCall as CorrectedCall  # noqa: E402

UNDECODABLE = P.SHAMIR_UNDECODABLE
PRIMES4 = (P17, P64, P255, SECP_N)


def pack(sets, count):
    """packed mask words [S][W] of the erased column sets, the padding bits of every second row set (they are ignored)"""
    W = (count + 63) // 64
    m = np.zeros((len(sets), W), dtype=np.uint64)
    for s, cols in enumerate(sets):
        for c in cols:
            m[s, c // 64] |= np.uint64(1 << (c % 64))
        if s % 2 and count % 64:
            m[s, W - 1] |= np.uint64(U64 ^ ((1 << (count % 64)) - 1))
    return m


def bits_of(mask, s, count):
    return [c for c in range(count) if (int(mask[s][c // 64]) >> (c % 64)) & 1]


def host_erasures(idx, rows, t, pm, er, layout="secret_major"):
    arr, (ss, ps) = laid_out(rows, layout)
    S, count = rows.shape[:2]
    ix = np.array(idx, dtype=np.uint64)
    W = (count + 63) // 64
    out, nerr, col, mask = (np.full((S, 4), 9, np.uint64), np.full(S, 9, np.uint32), np.full(count, 9, np.uint32),
                            np.full((S, W), 9, np.uint64))
    lib = _ffi.lib()
    api._check(lib.pvw_shamir_reconstruct_wide_erasures_host(nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(arr), S, ss, ps,
                                                             nptr(er), nptr(out), nptr(nerr), nptr(col), nptr(mask)), lib)
    return out, nerr, col, mask


class DeviceCall:
    """one pvw_shamir_reconstruct_wide_erasures_device call with its buffers kept (a captured call is replayed on them)"""

    def __init__(self, p, idx, rows, t, pm, er, layout="secret_major", nerr=True, col=True, mask=True):
        arr, (self.ss, self.ps) = laid_out(rows, layout)
        self.p, self.t, self.pm = p, t, api._wide_modulus(pm)
        self.S, self.count = rows.shape[:2]
        self.ix = np.array(idx, dtype=np.uint64)
        self.d_sh = dev(arr)
        self.d_er = None if er is None else dev(er)
        W = (self.count + 63) // 64
        self.out = torch.full((self.S, 4), -1, dtype=torch.int64, device=DEV)
        self.nerr = torch.full((self.S,), 9, dtype=torch.int32, device=DEV) if nerr else None
        self.col = torch.full((self.count,), 9, dtype=torch.int32, device=DEV) if col else None
        self.mask = torch.full((self.S, W), -1, dtype=torch.int64, device=DEV) if mask else None

    def enqueue(self, stream_ptr):
        return self.p._lib.pvw_shamir_reconstruct_wide_erasures_device(self.p._h, nptr(self.pm), self.t, nptr(self.ix), self.count,
                                                                       ptr(self.d_sh), self.S, self.ss, self.ps, ptr(self.d_er),
                                                                       ptr(self.out), ptr(self.nerr), ptr(self.col), ptr(self.mask),
                                                                       stream_ptr)

    def results(self):
        return (u64(self.out), None if self.nerr is None else self.nerr.cpu().numpy().view(np.uint32),
                None if self.col is None else self.col.cpu().numpy().view(np.uint32), None if self.mask is None else u64(self.mask))


def device_erasures(p, idx, rows, t, pm, er, layout, stream, **kw):
    call = DeviceCall(p, idx, rows, t, pm, er, layout, **kw)
    torch.cuda.synchronize()
    api._check(call.enqueue(C.c_void_p(stream.cuda_stream)), p._lib)
    stream.synchronize()
    return call.results()


def buffer_erasures(p, idx, rows, t, pm, er, layout):
    arr, _ = laid_out(rows, layout)
    out, nerr, col, mask = P.shamir_reconstruct_wide_corrected(p, idx, arr, t, pm, layout=layout, erased=er)
    return api._wide(out), nerr, col, mask


def classes(r, count):
    """(eps, nu) for eps in {0, 1, r - 1, r, r + 1} x nu in {0, E_s, E_s + 1} that fit into the row"""
    out = []
    for eps in sorted({e for e in (0, 1, r - 1, r, r + 1) if 0 <= e <= count}):
        Es = (r - eps) // 2 if eps <= r else 0
        out += [(eps, nu) for nu in sorted({0, Es, Es + 1}) if eps + nu <= count]
    return out


def plant(rows, plans, rng, junk=0):
    """a copy of rows: in row s the columns plans[s][0] erased and filled with junk (2^256 - 1, or random words), one bit flipped
    in the columns plans[s][1]"""
    bent = rows.copy()
    for s, (ers, errs) in enumerate(plans):
        for c in errs:
            bend(bent, s, c, rng)
        for k, c in enumerate(ers):
            bent[s, c] = np.uint64(U64) if (k + junk) % 2 == 0 else np.array([rng.getrandbits(64) for _ in range(4)], dtype=np.uint64)
    return bent


def plans_for(S, count, r, k, rng):
    """row s: a class in turn, or (every fifth row) a random mask with a random number of errors within the bound"""
    cl = classes(r, count)
    plans = []
    for s in range(S):
        if (s + k) % 5 == 4:
            eps = rng.randrange(r + 1)
            nu = rng.randrange((r - eps) // 2 + 1)
        else:
            eps, nu = cl[(s + k) % len(cl)]
        cols = rng.sample(range(count), eps + nu)
        plans.append((sorted(cols[:eps]), sorted(cols[eps:])))
    return plans


def check_planted(want, plans, secrets, r, count, pm, tag):
    for s, (ers, errs) in enumerate(plans):
        if len(ers) <= r and len(errs) <= (r - len(ers)) // 2:
            assert ints(want[0])[s] == secrets[s] and want[1][s] == len(errs), ("planted", tag, s)
            assert bits_of(want[3], s, count) == errs, ("planted bits", tag, s)
        elif len(ers) > r:
            assert want[1][s] == UNDECODABLE and not want[3][s].any() and not want[0][s].any(), ("eps > r", tag, s)
        assert not set(bits_of(want[3], s, count)) & set(ers), ("an erased column reported", tag, s)


def small(tp1):
    """device == host on all four outputs at t + 1 = tp1 and r in {0, 1, 2, 3, 8, 9, 63, 64, 65, 126 .. 130}: both sides of the mask
    word, of the 64-target block of either product, of the four-wave term split, of the 8-term chunk and of the 64-coefficient
    blocks of Gamma, the Forney pass and the locator; num_secrets 1 .. 9 in turn; both layouts; unreduced words; every class
    (eps, nu) in turn and random masks, each row its own; junk at the erased positions, and other junk changing nothing; NULL
    outputs; four primes in turn; the host-buffer form"""
    N = 170
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(300 + tp1)
    t = tp1 - 1
    k = tp1
    for r in (0, 1, 2, 3, 8, 9, 63, 64, 65, 126, 127, 128, 129, 130):
        count = tp1 + r
        S, pm = 1 + k % 9, PRIMES4[k % 4]
        k += 1
        idx, rows, secrets = sharing(p, N, S, t, pm, count, rng, tag=k)
        plans = plans_for(S, count, r, k, rng)
        bent = plant(rows, plans, rng)
        er = pack([e for e, _ in plans], count)
        want = host_erasures(idx, bent, t, pm, er)
        if pm > 2**64:
            check_planted(want, plans, secrets, r, count, pm, (tp1, r))
        for layout in ("secret_major", "party_major"):
            got = device_erasures(p, idx, bent, t, pm, er, layout, s)
            assert same(got, want), ("device", tp1, r, S, pm, layout, got[1], want[1])
        other = plant(rows, plans, random.Random(k), junk=1)     # other errors of the same columns would differ: only the junk moves
        for srow, (ers, _) in enumerate(plans):
            for c in range(count):
                if c not in ers:
                    other[srow, c] = bent[srow, c]
        assert same(device_erasures(p, idx, other, t, pm, er, "secret_major", s), want), ("junk", tp1, r)
        if k % 2 == 0 or r == 130:
            layout = ("secret_major", "party_major")[(k // 2) % 2]
            assert same(buffer_erasures(p, idx, bent, t, pm, er, layout), want), ("host-buffer", tp1, r, S, pm, layout)
        if k % 3 == 0:
            assert same(device_erasures(p, idx, bent, t, pm, er, "secret_major", s, nerr=False), want), ("no nerr", tp1, r)
            assert same(device_erasures(p, idx, bent, t, pm, er, "party_major", s, col=False, mask=False), want), ("no col_err, mask", tp1, r)
            assert same(device_erasures(p, idx, bent, t, pm, er, "secret_major", s, nerr=False, col=False, mask=False), want), ("out", tp1, r)
        print(f"small t+1={tp1} r={r} S={S} ok", flush=True)
    print(f"small {tp1} ok", flush=True)


def null():
    """a NULL mask is the wide corrected device call on every output, and an all-zero mask gives the same report by the other
    kernels; an err_mask fed back as the mask leaves no error"""
    N = 140
    p = _params(N)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(41)
    for S, t, count, pm in ((5, 3, 20, SECP_N), (9, 32, 100, P255), (2, 0, 67, P64)):
        r = count - t - 1
        idx, rows, secrets = sharing(p, N, S, t, pm, count, rng, tag=S)
        plans = [([], sorted(rng.sample(range(count), (0, 1, r // 2, r // 2 + 1)[srow % 4]))) for srow in range(S)]
        bent = plant(rows, plans, rng)
        for layout in ("secret_major", "party_major"):
            old = CorrectedCall(p, idx, bent, t, pm, layout)
            torch.cuda.synchronize()
            api._check(old.enqueue(C.c_void_p(s.cuda_stream)), p._lib)
            s.synchronize()
            base = old.results()
            assert same(device_erasures(p, idx, bent, t, pm, None, layout, s), base), ("NULL", S, layout)
            zero = np.zeros((S, (count + 63) // 64), dtype=np.uint64)
            assert same(device_erasures(p, idx, bent, t, pm, zero, layout, s), base), ("zero mask", S, layout)
            fed = device_erasures(p, idx, bent, t, pm, base[3], layout, s)
            for srow in range(S):
                if base[1][srow] != UNDECODABLE:
                    assert ints(fed[0])[srow] == secrets[srow] and fed[1][srow] == 0 and not fed[3][srow].any(), ("fed back", S, srow)
        assert same(buffer_erasures(p, idx, bent, t, pm, None, "secret_major"), base), ("host-buffer NULL", S)
    print("null ok", flush=True)


def far():
    """arbitrary words over p = 65537: far rows decode to polynomials nobody dealt, and the device finds what the host finds"""
    p = _params(7)
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(42)
    nrng = np.random.default_rng(42)
    decoded = 0
    for t, count, S in ((0, 3, 40), (1, 5, 40), (2, 6, 40), (1, 9, 24), (3, 8, 24)):
        r = count - t - 1
        idx = rng.sample(range(60000), count)
        rows = nrng.integers(0, 2**64, (S, count, 4), dtype=np.uint64)
        er = pack([rng.sample(range(count), srow % (r + 2)) for srow in range(S)], count)
        want = host_erasures(idx, rows, t, P17, er)
        decoded += int((want[1] != UNDECODABLE).sum())
        for layout in ("secret_major", "party_major"):
            assert same(device_erasures(p, idx, rows, t, P17, er, layout, s), want), (t, count, layout)
    assert decoded > 20, decoded
    print("far ok", flush=True)


def mask():
    """pvw_shamir_wide_erasure_mask_device == _host: counts either side of a word and of a wave's 64 words, NL in {1, 5, 16}, the
    three stride sets, either array alone, noise == noise_bound (not erased); through the Python wrapper on device tensors"""
    p = _params(7)
    s = torch.cuda.Stream(device=DEV)
    lib = _ffi.lib()
    nrng = np.random.default_rng(43)
    for NL in (1, 5, 16):
        for count in (1, 63, 64, 65, 4095, 4096, 4097):
            S = 3 if count < 4000 else 2
            n = S * count * NL
            st = (nrng.integers(1, 16, n, dtype=np.uint32) * (nrng.random(n) < 0.05)).astype(np.uint32)
            nz = nrng.integers(0, 1000, n, dtype=np.uint64)
            nz[nrng.random(n) < 0.01] = np.uint64(U64)
            d_st, d_nz = dev(st.view(np.int32)), dev(nz)
            for strides in ((count * NL, NL, 1), (NL, S * NL, 1), (count, 1, S * count)):
                for a, b, da, db in ((st, nz, d_st, d_nz), (st, None, d_st, None), (None, nz, None, d_nz)):
                    bits, bound = (4, 998) if strides[2] == 1 else (0xFFFFFFFF, 999)
                    want = np.full((S, (count + 63) // 64), 5, dtype=np.uint64)
                    api._check(lib.pvw_shamir_wide_erasure_mask_host(nptr(a), nptr(b), bits, bound, count, S, strides[0], strides[1], NL,
                                                                     strides[2], nptr(want)), lib)
                    got = torch.full(want.shape, -1, dtype=torch.int64, device=DEV)
                    torch.cuda.synchronize()
                    p._call("pvw_shamir_wide_erasure_mask_device", ptr(da), ptr(db), bits, bound, count, S, strides[0], strides[1], NL,
                            strides[2], ptr(got), C.c_void_p(s.cuda_stream))
                    s.synchronize()
                    assert np.array_equal(u64(got), want), (NL, count, strides, a is None, b is None)
                    if NL == 1:
                        one = torch.full(want.shape, -1, dtype=torch.int64, device=DEV)
                        p._call("pvw_shamir_erasure_mask_device", ptr(da), ptr(db), bits, bound, count, S, strides[0], strides[1], ptr(one),
                                C.c_void_p(s.cuda_stream))
                        s.synchronize()
                        assert np.array_equal(u64(one), want), ("one-word builder", count, strides)
            t_mask = P.shamir_wide_erasure_mask(d_st.view(count, S * NL), d_nz.view(count, S * NL), num_limbs=NL, status_bits=4,
                                                noise_bound=998, layout="party_major", params=p, stream=s)
            s.synchronize()
            want = P.shamir_wide_erasure_mask(st.reshape(count, S * NL), nz.reshape(count, S * NL), num_limbs=NL, status_bits=4,
                                              noise_bound=998, layout="party_major", host=True)
            assert np.array_equal(u64(t_mask), want) and (want.any() or count == 1), (NL, count)
    print("mask ok", flush=True)


def planted(count, t, S, pm, rng):
    idx = rng.sample(range(1 << 40), count)
    polys = [[rng.randrange(pm) for _ in range(t + 1)] for _ in range(S)]
    vals = [[sum(a[j] * pow(i + 1, j, pm) for j in range(t + 1)) % pm for i in idx] for a in polys]
    return idx, polys, vals


def run_planted(p, s, idx, polys, vals, plans, t, pm, expect_ok):
    """rows of planted erasures (junk) and errors (uniformly random other values) through the device form: a row within the bound
    comes back exactly, a row beyond it is undecodable (the argument of the wide corrected worker's lds() on the sub-row)"""
    S, count = len(vals), len(idx)
    vals = [list(v) for v in vals]
    for srow, (ers, errs) in enumerate(plans):
        for c in errs:
            vals[srow][c] = (vals[srow][c] + 1 + rng_planted.randrange(pm - 1)) % pm
        for c in ers:
            vals[srow][c] = U64 if c % 2 else rng_planted.getrandbits(256)
    rows = words([v for row in vals for v in row], (S, count))
    er = pack([e for e, _ in plans], count)
    out, nerr, col, mask = device_erasures(p, idx, rows, t, pm, er, "secret_major", s)
    want_col = np.zeros(count, np.uint32)
    for srow, (ers, errs) in enumerate(plans):
        if expect_ok[srow]:
            assert ints(out)[srow] == polys[srow][0] and nerr[srow] == len(errs), ("planted", srow, nerr[srow])
            assert bits_of(mask, srow, count) == sorted(errs), ("bits", srow)
            want_col[list(errs)] += 1
        else:
            assert ints(out)[srow] == 0 and nerr[srow] == UNDECODABLE and not mask[srow].any(), ("beyond", srow, nerr[srow])
    assert np.array_equal(col, want_col)


rng_planted = random.Random(44)


def lds(which):
    """The dynamic-LDS opt-in path against planted truth (the cubic host form is not run at these sizes).
    lo: count 2053, t 2, r 2050: (r + 3) 32 = 65 696 bytes, above the 64 KiB a launch gets without asking, 1025 erased and 512
    overwritten (2 * 512 + 1025 = 2049 <= r).
    hi: count 4098, t 2, r 4095, the bound: 131 136 bytes; S = 2, row 0 with 4095 erased, row 1 with 2047 erased + 1024
    overwritten (2 * 1024 + 2047 = 4095); then one more bad column in either row: 4096 erased (eps > r), and 2047 erased + 1025
    overwritten, which must both be PVW_SHAMIR_UNDECODABLE."""
    rng = random.Random(45)
    p = _params(7)
    s = torch.cuda.Stream(device=DEV)
    pm, t = SECP_N, 2
    if which == "lo":
        count = 2053
        assert (count - t - 1 + 3) * 32 == 65696 > 65536
        idx, polys, vals = planted(count, t, 1, pm, rng)
        cols = rng.sample(range(count), 1025 + 512)
        run_planted(p, s, idx, polys, vals, [(cols[:1025], cols[1025:])], t, pm, [True])
    else:
        count = 4098
        assert (count - t - 1 + 3) * 32 == 131136
        idx, polys, vals = planted(count, t, 2, pm, rng)
        a = rng.sample(range(count), 4096)
        b = rng.sample(range(count), 2047 + 1025)
        run_planted(p, s, idx, polys, vals, [(a[:4095], []), (b[:2047], b[2047:2047 + 1024])], t, pm, [True, True])
        run_planted(p, s, idx, polys, vals, [(a, []), (b[:2047], b[2047:])], t, pm, [False, False])
    print(f"lds {which} ok", flush=True)


def pieces():
    """the host-buffer form through both copy paths (dense rows by a 2D copy, party-major by a host repack) in several staged
    pieces, and the device form in several passes (the tuning build with a small PVW_STAGE_BYTES / PVW_CORRECT_PIECE_BYTES): all
    equal the host routine, col_err summed over the pieces, every piece with its own mask rows; nothing secret is left behind
    after success nor after a refusal"""
    _ffi.select("tuning")
    for name in ("PVW_STAGE_BYTES", "PVW_CORRECT_PIECE_BYTES"):
        os.environ.pop(name, None)
    N, S, t, count, pm = 100, 23, 6, 40, SECP_N
    r = count - t - 1
    p = _params(N)
    assert p._lib.pvw_build_is_tuning() == 1
    s = torch.cuda.Stream(device=DEV)
    rng = random.Random(46)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plans = plans_for(S, count, r, 0, rng)
    for ers, errs in plans:
        if len(ers) + 2 * len(errs) + 2 <= r and count - 2 not in ers and count - 2 not in errs:
            errs.append(count - 2)                                  # a bent column: every piece adds to col_err
            errs.sort()
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    want = host_erasures(idx, bent, t, pm, er)
    assert want[2][count - 2] >= 5 and (want[1] == UNDECODABLE).any() and (want[1] == 0).any()
    for layout in ("secret_major", "party_major"):                 # one piece, one pass
        assert same(buffer_erasures(p, idx, bent, t, pm, er, layout), want), layout
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= (S * count + S + S * count) * 4, ("residue", layout, nz, scanned)
    item = (count + 1) * 32 + 2 * 8 + 4
    os.environ["PVW_STAGE_BYTES"] = str(5 * item + 7)               # 5 secrets a piece: 4 full pieces and one of 3
    try:
        for layout in ("secret_major", "party_major"):
            assert same(buffer_erasures(p, idx, bent, t, pm, er, layout), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_STAGE_BYTES", None)
    per = (count + r + r + 1) * 32 + 4
    os.environ["PVW_CORRECT_PIECE_BYTES"] = str(4 * per + 3)        # 4 secrets a pass: 5 full passes and one of 3
    try:
        for layout in ("secret_major", "party_major"):
            assert same(device_erasures(p, idx, bent, t, pm, er, layout, s), want), layout
            assert same(buffer_erasures(p, idx, bent, t, pm, er, layout), want), layout
            assert api._secret_residue(p)[0] == 0
    finally:
        os.environ.pop("PVW_CORRECT_PIECE_BYTES", None)
    # a refused call leaves nothing behind and writes nothing
    ix = np.array(idx, dtype=np.uint64)
    ix[3] = ix[0]
    out = np.zeros((S, 4), np.uint64)
    rc = p._lib.pvw_shamir_reconstruct_wide_erasures(p._h, nptr(api._wide_modulus(pm)), t, nptr(ix), count, nptr(bent), S, count, 1, nptr(er),
                                                     nptr(out), None, None, None)
    assert rc == INVALID_PARAMETERS and "duplicate" in _ffi.last_error(p._lib) and not out.any()
    assert api._secret_residue(p)[0] == 0
    print("pieces ok", flush=True)


def capture():
    """under stream capture on a stream that only a maskless call has sized, the call with a mask is refused with its own error
    and the capture survives empty; after one sizing call with a mask outside capture a captured call replays, and every replay
    reports on the shares and on the MASK that are in the buffers then"""
    N, S, t, count, pm = 140, 9, 40, 110, SECP_N
    r = count - t - 1
    rng = random.Random(47)
    p = _params(N)
    idx, rows, _ = sharing(p, N, S, t, pm, count, rng)
    plans = plans_for(S, count, r, 1, rng)
    bent = plant(rows, plans, rng)
    er = pack([e for e, _ in plans], count)
    want = host_erasures(idx, bent, t, pm, er)
    call = DeviceCall(p, idx, bent, t, pm, er)
    s0 = torch.cuda.Stream(device=DEV)
    old = CorrectedCall(p, idx, bent, t, pm)
    torch.cuda.synchronize()
    api._check(old.enqueue(C.c_void_p(s0.cuda_stream)), p._lib)     # sizes the stream's workspace for the maskless call only
    s0.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc = call.enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = _ffi.last_error(p._lib)
    torch.cuda.synchronize()
    assert rc == INVALID_PARAMETERS and "capture" in msg and "erasure mask" in msg, (rc, msg)
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
        # new shares at the SAME points and another mask: the captured call carries the indices it was made with
        full = P.shamir_shares_wide(p, [rng.getrandbits(256) for _ in range(S)], t, pm, seeds=seeds_for(S, tag=50 + rep), host=True)
        plans2 = plans_for(S, count, r, 2 + 3 * rep, rng)
        fresh = plant(np.ascontiguousarray(full[:, idx]), plans2, rng)
        er2 = pack([e for e, _ in plans2], count)
        call.d_sh.copy_(dev(fresh))
        call.d_er.copy_(dev(er2))
        call.out.fill_(-1), call.nerr.fill_(9), call.col.fill_(9), call.mask.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want2 = host_erasures(idx, fresh, t, pm, er2)
        assert (want2[1] == UNDECODABLE).any() and (want2[1] != UNDECODABLE).any() and not np.array_equal(er2, er)
        assert same(call.results(), want2), rep
    del g
    print("capture ok", flush=True)


def concurrent():
    """the promise of include/pvw_hip.h for pvw_shamir_reconstruct_wide_erasures: two threads on one context overlap calls of
    different shapes, every result equals the serial one bit for bit, nothing is left in a workspace"""
    N = 140
    p = _params(N)
    rng = random.Random(48)
    jobs = []
    for k, (S, t, count, pm) in enumerate(((5, 4, 12, SECP_N), (20, 20, 90, P255), (7, 9, 77, P64), (12, 3, 40, P17))):
        idx, rows, _ = sharing(p, N, S, t, pm, count, rng, tag=k)
        plans = plans_for(S, count, count - t - 1, k, rng)
        bent = plant(rows, plans, rng)
        er = pack([e for e, _ in plans], count)
        layout = ("secret_major", "party_major")[k % 2]
        jobs.append(lambda idx=idx, bent=bent, t=t, pm=pm, er=er, layout=layout: buffer_erasures(p, idx, bent, t, pm, er, layout))
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
    """the whole chain on the device over the secp256k1 order at n = 9, t = 2 (r = 6), D = 4 dealers: deal
    (deal_party_shares_wide) -> c2 of five parties tampered for every dealer, each in a different limb ciphertext (another scalar's
    encoding and 2^70 on one coefficient added: another value, and a saturated noise in the report) ->
    pvw_decrypt_all_checked_device, [party][dealer NL + w] -> pvw_shamir_wide_erasure_mask_device on that report in place, strides
    (NL, D NL, 1) -> the fold in place -> reconstruction in place, strides (1, D), every dealer a secret.  Five bad shares a row
    are more than E = 3, so the wide corrected call reports every row undecodable; as erasures (5 <= r) every secret comes back
    with nerr = 0."""
    rng = random.Random(49)
    n, k, l, D, t, pm, lb = 9, 32, 8, 4, 2, SECP_N, 52
    p, gpk, parties = system(n, k, l, M.bench_moduli(5))
    nl = P.shamir_wide_limbs(pm, lb)
    assert nl == 5
    V = D * nl
    secrets = [pm - 1 - rng.randrange(1 << 100) for _ in range(D)]
    cts = P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds_for(V, tag=11), limb_bits=lb)
    assert len(cts) == D and all(len(row) == nl for row in cts)
    cts = [ct for row in cts for ct in row]                          # vector d * NL + w
    tampered = [sorted(rng.sample(range(n), 5)) for _ in range(D)]
    e = np.zeros((p.L, p.l), dtype=np.uint64)
    e[:, 1] = [(1 << 70) % q for q in p.moduli()]
    bump = p.ntt_forward(e).astype(object) + p.encode_scalar(12345, P.REPR_NTT).astype(object)
    qq = np.array(p.moduli(), dtype=object)[:, None]
    for d in range(D):
        for j, party in enumerate(tampered[d]):                    # party j of the five in limb j
            ct = cts[d * nl + j]
            ct.c2[party] = ((ct.c2[party].astype(object) + bump) % qq).astype(np.uint64)
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
    out = torch.zeros((D, 4), dtype=torch.int64, device=DEV)
    nerr = torch.full((D,), 9, dtype=torch.int32, device=DEV)
    col = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    emask = torch.full((D, 1), -1, dtype=torch.int64, device=DEV)
    cout = torch.zeros((D, 4), dtype=torch.int64, device=DEV)
    cnerr = torch.full((D,), 9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p._call("pvw_decrypt_all_checked_device", 0, n, ptr(d_sk), ptr(c1), ptr(c2), V, P.REPR_NTT, ptr(limbs), ptr(noise), ptr(status), sp)
    p._call("pvw_shamir_wide_erasure_mask_device", ptr(status), ptr(noise), P.DEC_LOSSY, p.noise_bound(), n, D, nl, V, nl, 1, ptr(d_mask), sp)
    folded = P.shamir_wide_from_limbs_device(p, limbs, pm, lb, layout="limb_minor", num_limbs=nl, stream=s)   # [n * D][4]
    p._call("pvw_shamir_reconstruct_wide_erasures_device", nptr(pmw), t, nptr(idx), n, ptr(folded), D, 1, D, ptr(d_mask), ptr(out),
            ptr(nerr), ptr(col), ptr(emask), sp)
    p._call("pvw_shamir_reconstruct_wide_corrected_device", nptr(pmw), t, nptr(idx), n, ptr(folded), D, 1, D, ptr(cout), ptr(cnerr), None,
            None, sp)
    s.synchronize()
    assert np.array_equal(u64(d_mask), pack(tampered, n) & np.uint64((1 << n) - 1)), "the checked decrypt flags exactly the tampered shares"
    assert cnerr.cpu().numpy().view(np.uint32).tolist() == [UNDECODABLE] * D, "five bad shares are beyond E = 3"
    assert ints(u64(out)) == secrets and nerr.cpu().tolist() == [0] * D
    assert not col.any().item() and not emask.any().item()
    print("loop ok", flush=True)


CASES = {f.__name__: f for f in (null, far, mask, pieces, capture, concurrent, loop)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    if sys.argv[1].startswith("small"):
        small(int(sys.argv[1][5:]))
    elif sys.argv[1].startswith("lds"):
        lds(sys.argv[1][3:])
    else:
        CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_ERASURES_OK")

"""Packed Shamir dealing over a prime field of up to 256 bits on the device: shamir_eval_packed_wide_kernel and the
weights kernels against pvw_shamir_shares_packed_wide_host, the fused deal against pvw_encrypt_multi of the host shares' limb
planes, pack = 1 against the wide calls, the _rs forms and stream capture, the loop closed down to the corrected sums of the
dealers' secrets, key hygiene, the host-buffer forms in pieces and from several threads.  Everything is bit for bit.  torch is
imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_packed_wide.py; prints
SHAMIR_PACKED_WIDE_OK."""
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
from _util import EXAMPLE_MODULI  # noqa: E402
from test_shamir_wide_host import SECP_N, ints, seeds_for  # noqa: E402
from _shamir_wide_worker import (DEV, S, _params, deal_device as wide_deal_device, dev, flat, ptr, same, seed_bytes, system, u64,  # noqa: E402
                                 unreduced)

P17, P64, P255 = 65537, 2**64 + 13, 2**255 - 19
PRIMES4 = (P17, P64, P255, SECP_N)
SHW_JC = 256                        # the kernel's staging chunk, in Horner terms and in secrets


def packed_secrets(pm, rng, D, K):
    flat_ = unreduced(pm, rng, D * K)
    return [flat_[d * K:(d + 1) * K] for d in range(D)]


def device_shares(p, secrets, K, t, pm, seeds=None, coeffs=None, stream=None, fill=0):
    """pvw_shamir_shares_packed_wide_device on `stream`: the (D, n, 4) buffer, pre-filled with `fill`"""
    D = len(secrets)
    out = torch.full((D, p.n, 4), fill, dtype=torch.int64, device=DEV)
    d_se = dev(api._wide_packed_secrets(secrets, K))
    d_co = None if coeffs is None or t == 0 else dev(api._wide([v for row in coeffs for v in row]))
    sd = None if seeds is None else seed_bytes(seeds)
    s = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    p._call("pvw_shamir_shares_packed_wide_device", ptr(d_se), D, K, t, api._ptr(api._wide_modulus(pm)), api._ptr(sd), ptr(d_co), ptr(out),
            C.c_void_p(s.cuda_stream))
    s.synchronize()
    return u64(out)


def check_shares(p, rng, s, D, K, t, pm, tag, explicit=True, host_buffer=False):
    secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(D, tag=t + K)
    want = P.shamir_shares_packed_wide(p, secrets, K, t, pm, seeds=seeds if t else None, host=True)
    assert np.array_equal(device_shares(p, secrets, K, t, pm, seeds=seeds if t else None, stream=s), want), ("drawn",) + tag
    if host_buffer:
        assert np.array_equal(P.shamir_shares_packed_wide(p, secrets, K, t, pm, seeds=seeds), want), ("host-buffer",) + tag
    if t and explicit:
        coeffs = [unreduced(pm, rng, t)] + [[rng.getrandbits(256) for _ in range(t)] for _ in range(D - 1)]
        want = P.shamir_shares_packed_wide(p, secrets, K, t, pm, coeffs=coeffs, host=True)
        assert np.array_equal(device_shares(p, secrets, K, t, pm, coeffs=coeffs, stream=s), want), ("explicit",) + tag
        if host_buffer:
            assert np.array_equal(P.shamir_shares_packed_wide(p, secrets, K, t, pm, coeffs=coeffs), want), ("explicit host-buffer",) + tag
    if K == 1:                                                       # the wide call it extends
        assert np.array_equal(want, P.shamir_shares_wide(p, [r[0] for r in secrets], t, pm, seeds=seeds if t and not explicit else None,
                                                         coeffs=coeffs if t and explicit else None, host=True)), ("pack 1",) + tag


def shares():
    """device shares == host shares, bit for bit: n = 3, 70, 300; K = 1, 2, 5, 64 and the secret chunk's edge 255 .. 257 at n = 300;
    t = 0, 1 and the Horner chunk's edge 254 .. 257 at K = 5; D = 1, 5 and 130 (three launches); four primes; drawn and explicit
    coefficients, unreduced words; device-pointer and host-buffer forms; sharded contexts that start off a multiple of 256"""
    rng = random.Random(1)
    s = torch.cuda.Stream(device=DEV)
    for n in (3, 70, 300):
        p = _params(n)
        for K in (1, 2, 5, 64):
            if K > n:
                continue
            for t in sorted({0, 1, min(7, n - K), n - K}):
                if t + K > n:
                    continue
                for i, pm in enumerate(PRIMES4):
                    if n == 300 and t != 1 and pm in (P64, P255):
                        continue
                    check_shares(p, rng, s, 5 if i == 3 else 1, K, t, pm, (n, K, t, pm), host_buffer=(i == 3))
        print(f"shares n={n} ok", flush=True)
    p = _params(300)
    for K in (255, 256, 257):                                        # the secret chunk edge
        for pm in (P64, SECP_N):
            check_shares(p, rng, s, 2, K, 3, pm, ("secret chunk", K, pm), explicit=False)
    for t in (254, 255, 256, 257):                                   # the Horner chunk edge
        for pm in (P17, SECP_N):
            check_shares(p, rng, s, 2, 5, t, pm, ("horner chunk", t, pm))
    print("shares chunk edges ok", flush=True)
    p = _params(70)
    check_shares(p, rng, s, 130, 5, 9, P255, ("three launches",), explicit=False, host_buffer=True)
    print("shares three launches ok", flush=True)
    # sharded: columns [party_lo, party_hi) are written, the others keep what the buffer held
    n, D, K, t, pm = 300, 5, 5, 77, SECP_N
    full = _params(n)
    secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(D)
    want = P.shamir_shares_packed_wide(full, secrets, K, t, pm, seeds=seeds, host=True)
    marker = np.uint64((1 << 64) - 7)
    for lo, hi in ((37, 295), (257, 300), (1, 2)):
        part = _params(n, shard=(lo, hi, 0, 1))
        got = device_shares(part, secrets, K, t, pm, seeds=seeds, stream=s, fill=-7)
        assert np.array_equal(got[:, lo:hi], want[:, lo:hi]) and (got[:, :lo] == marker).all() and (got[:, hi:] == marker).all(), (lo, hi)
        hb = P.shamir_shares_packed_wide(part, secrets, K, t, pm, seeds=seeds)
        assert np.array_equal(hb[:, lo:hi], want[:, lo:hi]) and not hb[:, :lo].any() and not hb[:, hi:].any(), (lo, hi)
    print("shares shard ok", flush=True)


def limb_planes(p, secrets, K, t, pm, seeds, limb_bits):
    """the scalars of the D * NL vectors: row d * NL + w is limb w of dealer d's host shares, drawn under seeds[d * NL]"""
    nl = P.shamir_wide_limbs(pm, limb_bits)
    sh = P.shamir_shares_packed_wide(p, secrets, K, t, pm, seeds=seeds[::nl], host=True)
    return np.concatenate([P.shamir_wide_to_limbs(sh[d], limb_bits, nl) for d in range(len(secrets))]), nl


def two_step(p, gpk, secrets, K, t, pm, seeds, limb_bits, repr):
    rows, _ = limb_planes(p, secrets, K, t, pm, seeds, limb_bits)
    return P.encrypt_many(rows.tolist(), gpk, seeds, repr)


def deal_device(p, secrets, K, t, pm, limb_bits, repr, stream, seeds=None, st=None):
    D = len(secrets)
    V = D * P.shamir_wide_limbs(pm, limb_bits)
    rA, rB = p.c1_hi - p.c1_lo, p.party_hi - p.party_lo
    c1 = torch.zeros((V, rA, p.L, p.l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((V, rB, p.L, p.l), dtype=torch.int64, device=DEV)
    d_se = dev(api._wide_packed_secrets(secrets, K))
    pmw = api._ptr(api._wide_modulus(pm))
    torch.cuda.synchronize()
    if st is None:
        p._call("pvw_deal_shares_packed_wide_device", ptr(d_se), D, K, t, pmw, limb_bits, api._ptr(seed_bytes(seeds)), ptr(c1), ptr(c2), repr,
                C.c_void_p(stream.cuda_stream))
    else:
        p._call("pvw_deal_shares_packed_wide_rs_device", ptr(d_se), D, K, t, pmw, limb_bits, st._h, ptr(c1), ptr(c2), repr,
                C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(c1), u64(c2)


def deal():
    """pvw_deal_shares_packed_wide[_device] == pvw_encrypt_multi of the host shares' limb planes under the same seeds, bit for bit:
    D * NL = 2 (VALU) and 5, 10, 135 (matrix cores; 135 is more than one pass of 128, with a dealer's limbs on both sides of the
    cut), NTT and power output, 52- and 62-bit limbs, host-buffer and device-pointer forms, a sharded context; pack = 1 gives the
    ciphertexts of pvw_deal_shares_wide*"""
    rng = random.Random(3)
    s = torch.cuda.Stream(device=DEV)
    n, k, l = 40, 64, 8
    for name, moduli in (("17x61", M.bench_moduli(17)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, _ = system(moduli, n, k, l)
        for D, K, pm, lb, repr, t in ((1, 3, 2**89 - 1, 52, P.REPR_NTT, n - 3), (1, 2, SECP_N, 62, P.REPR_POWER, 7), (2, 5, SECP_N, 52, P.REPR_NTT, 7),
                                      (2, 1, SECP_N, 62, P.REPR_POWER, n - 1), (27, 4, SECP_N, 52, P.REPR_NTT, 7)):
            if D >= 27 and name != "17x61":
                continue
            nl = P.shamir_wide_limbs(pm, lb)
            secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(D * nl, tag=D)
            want = two_step(p, gpk, secrets, K, t, pm, seeds, lb, repr)
            got = flat(P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, seeds=seeds, limb_bits=lb, out_repr=repr))
            assert same(got, want), ("host-buffer", name, D, nl, repr)
            g1, g2 = deal_device(p, secrets, K, t, pm, lb, repr, s, seeds=seeds)
            for v in range(D * nl):
                assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("device", name, D, nl, repr, v)
            if K == 1:
                w1, w2 = wide_deal_device(p, [r[0] for r in secrets], t, pm, lb, repr, s, seeds=seeds)
                assert np.array_equal(g1, w1) and np.array_equal(g2, w2), ("pack 1", name)
                assert same(got, flat(P.deal_party_shares_wide([r[0] for r in secrets], t, pm, gpk, seeds=seeds, limb_bits=lb, out_repr=repr)))
        print(f"deal {name} ok", flush=True)
    # sharded: ragged party and CRS-row ranges, both sides of the dispatch
    n, k = 70, 64
    moduli = M.bench_moduli(3)
    full, gfull, _ = system(moduli, n, k, l)
    part, gpart, _ = system(moduli, n, k, l, (13, 51, 16, 61))
    for D, K, pm, lb in ((1, 4, 2**89 - 1, 52), (2, 3, SECP_N, 52)):
        nl = P.shamir_wide_limbs(pm, lb)
        secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(D * nl, tag=40 + D)
        want = two_step(full, gfull, secrets, K, 33, pm, seeds, lb, P.REPR_NTT)
        g1, g2 = deal_device(part, secrets, K, 33, pm, lb, P.REPR_NTT, s, seeds=seeds)
        for v in range(D * nl):
            assert np.array_equal(g1[v], want[v].c1[16:61]) and np.array_equal(g2[v], want[v].c2[13:51]), ("shard device", D, v)
        got = flat(P.deal_party_shares_packed_wide(secrets, K, 33, pm, gpart, seeds=seeds, limb_bits=lb))
        for v in range(D * nl):
            assert np.array_equal(got[v].c1[16:61], want[v].c1[16:61]) and np.array_equal(got[v].c2[13:51], want[v].c2[13:51]), ("shard host", D, v)
    print("deal shard ok", flush=True)


def rs():
    """the _rs forms with state (S, c) equal the seeded forms with seeds call_seed(S, c + v) and leave c + D NL; under stream
    capture the call is refused without pvw_prepare, and after it without an earlier packed wide call of at least this size on the
    stream, with the error of pvw_encrypt_multi_device and the capture intact; sized, captured and replayed twice, the replays
    are the seeded deals of the counters they met: two fresh sharings"""
    lib = _ffi.lib()
    rng = random.Random(4)
    n, k, l, t, lb, K = 24, 32, 8, 5, 52, 3
    p, gpk, parties = system(M.bench_moduli(5), n, k, l, keys=True)
    s = torch.cuda.Stream(device=DEV)
    c = 77
    cseed = lambda x: P.DeviceRandomness.call_seed(S, x)
    with P.DeviceRandomness(p, S, c) as st:
        for D, pm in ((1, 2**89 - 1), (3, SECP_N)):
            nl = P.shamir_wide_limbs(pm, lb)
            V = D * nl
            secrets = packed_secrets(pm, rng, D, K)
            want = two_step(p, gpk, secrets, K, t, pm, [cseed(c + v) for v in range(V)], lb, P.REPR_NTT)
            g1, g2 = deal_device(p, secrets, K, t, pm, lb, P.REPR_NTT, s, st=st)
            for v in range(V):
                assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("rs device", D, v)
            c += V
            assert st.counter(s) == c, (D, st.counter(s))
            want = two_step(p, gpk, secrets, K, t, pm, [cseed(c + v) for v in range(V)], lb, P.REPR_POWER)
            got = flat(P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, randomness=st, limb_bits=lb, out_repr=P.REPR_POWER))
            assert same(got, want), ("rs host", D)
            c += V
            assert st.counter() == c, D
        print("rs forms ok", flush=True)
        ref_p, ref_gpk, ref_parties = system(M.bench_moduli(5), n, k, l, keys=True)
        for D, pm in ((1, 2**89 - 1), (2, SECP_N)):            # VALU path and matrix cores
            nl = P.shamir_wide_limbs(pm, lb)
            V = D * nl
            pmw = api._wide_modulus(pm)
            secrets = [[rng.randrange(pm) for _ in range(K)] for _ in range(D)]
            d_se = dev(api._wide_packed_secrets(secrets, K))
            c1 = torch.zeros((V, k, p.L, l), dtype=torch.int64, device=DEV)
            c2 = torch.zeros((V, n, p.L, l), dtype=torch.int64, device=DEV)
            enqueue = lambda cs, pack=K: lib.pvw_deal_shares_packed_wide_rs_device(p._h, ptr(d_se), D, pack, t, api._ptr(pmw), lb, st._h, ptr(c1),
                                                                                 ptr(c2), P.REPR_NTT, cs)

            def refused(stream):
                torch.cuda.synchronize()
                g0 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g0, stream=stream):
                    rc = enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    msg = _ffi.last_error(lib)
                torch.cuda.synchronize()
                del g0
                return rc, msg

            rc, msg = refused(torch.cuda.Stream(device=DEV))      # a stream the context has never seen
            assert rc == 1 and "pvw_prepare" in msg, (D, rc, msg)
            s1 = torch.cuda.Stream(device=DEV)
            p.prepare(P.PREPARE_MFMA, s1.cuda_stream)
            rc, msg = refused(s1)                                  # prepared, but no packed wide call has sized the weights
            assert rc == 1 and "packed wide call" in msg, (D, rc, msg)
            small = [row[:1] for row in secrets]                   # sized for pack 1 only: still refused
            d_small = dev(api._wide_packed_secrets(small, 1))
            api._check(lib.pvw_deal_shares_packed_wide_rs_device(p._h, ptr(d_small), D, 1, t, api._ptr(pmw), lb,
                                                                 st._h, ptr(c1), ptr(c2), P.REPR_NTT, C.c_void_p(s1.cuda_stream)), lib)
            s1.synchronize()
            c += V
            rc, msg = refused(s1)
            assert rc == 1 and "packed wide call" in msg, (D, rc, msg)
            assert st.counter(s) == c
            api._check(enqueue(C.c_void_p(s1.cuda_stream)), lib)   # outside capture: sizes the weights
            s1.synchronize()
            c += V
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s1):
                rc = enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
            api._check(rc, lib)
            seen = []
            for rep in range(2):
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                g1, g2 = u64(c1).copy(), u64(c2).copy()
                assert api._secret_residue(p)[0] == 0, ("residue after replay", D, rep)
                want = two_step(ref_p, ref_gpk, secrets, K, t, pm, [cseed(c + v) for v in range(V)], lb, P.REPR_NTT)
                for v in range(V):
                    assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("replay", D, rep, v)
                c += V
                seen.append((g1, g2))
            assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1]), D
            assert st.counter(s1) == c, D
            del g
        print("rs capture ok", flush=True)


def loop():
    """the loop closed over the secp256k1 order: five dealers deal three secrets each, the ciphertexts are summed limb by limb,
    every party decrypts its limb sums, folds them back mod p on the device, and the corrected packed reconstruction gives
    sum_d s_{d,j} mod p for every j -- clean, and with two parties' sums overwritten"""
    rng = random.Random(5)
    n, k, l, D, t, K, pm, lb = 12, 32, 8, 5, 3, 3, SECP_N, 52
    p, gpk, parties = system(M.bench_moduli(5), n, k, l, keys=True)
    nl = P.shamir_wide_limbs(pm, lb)
    secrets = [[pm - 1 - rng.randrange(1 << 100) for _ in range(K)] for _ in range(D)]
    cts = P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, seeds=seeds_for(D * nl, tag=9), limb_bits=lb)
    sums = []
    for w in range(nl):
        agg = P.aggregate_ciphertexts([cts[d][w] for d in range(D)])
        sums.append([int(v) for v in P.decrypt_all_party_sums([agg], parties).values])
    limbs = torch.tensor(sums, dtype=torch.int64, device=DEV)
    folded = u64(P.shamir_wide_from_limbs_device(p, limbs, pm, lb)).reshape(1, n, 4)
    want = [sum(secrets[d][j] for d in range(D)) % pm for j in range(K)]
    idx = list(range(n))
    rng.shuffle(idx)
    rows = np.ascontiguousarray(folded[:, idx, :])
    sec, nerr, col_err, mask = P.shamir_reconstruct_packed_wide_corrected(p, pm, K, t, idx, rows)
    assert sec == [want] and int(nerr[0]) == 0 and not col_err.any(), (sec, nerr)
    bent = rows.copy()
    bent[0, 1] = np.array([7, 7, 7, 7], dtype=np.uint64)
    bent[0, 8] ^= np.uint64(1 << 40)
    sec, nerr, col_err, mask = P.shamir_reconstruct_packed_wide_corrected(p, pm, K, t, idx, bent)
    assert sec == [want] and int(nerr[0]) == 2 and col_err.tolist() == [1 if c in (1, 8) else 0 for c in range(n)], (sec, nerr, col_err)
    assert int(mask[0, 0]) == (1 << 1) | (1 << 8)
    erased = np.zeros((1, n), dtype=bool)
    erased[0, 1] = True
    sec, nerr, _, _ = P.shamir_reconstruct_packed_wide_corrected(p, pm, K, t, idx, bent, erased=erased)
    assert sec == [want] and int(nerr[0]) == 1
    print("loop ok", flush=True)


def hygiene():
    """pvw_selftest_secret_residue reports zero after a host-buffer deal, a device-pointer deal once its stream is drained (both
    sides of the dispatch) and the host-buffer share call; the scanned regions are not empty"""
    rng = random.Random(6)
    n, k, l, t, lb, K = 40, 64, 8, 20, 52, 4
    p, gpk, _ = system(M.bench_moduli(3), n, k, l)
    s = torch.cuda.Stream(device=DEV)
    for D, pm in ((1, 2**89 - 1), (2, SECP_N), (27, SECP_N)):
        nl = P.shamir_wide_limbs(pm, lb)
        V = D * nl
        secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(V)
        P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, seeds=seeds, limb_bits=lb)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= min(V, 128) * n, ("host-buffer", D, nz, scanned)
        deal_device(p, secrets, K, t, pm, lb, P.REPR_NTT, s, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= min(V, 128) * n, ("device", D, nz, scanned)
        P.shamir_shares_packed_wide(p, secrets, K, t, pm, seeds=seeds[:D])
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= D * n * 4, ("shares", D, nz, scanned)
    print("hygiene ok", flush=True)


def pieces():
    """the host-buffer forms staged in more than one piece (the measurement build's PVW_STAGE_BYTES): the shares at D = 7 in
    pieces of 3 dealers, drawn and explicit; the deal at D = 5 in pieces of 2 whole dealers, seeded and from a randomness state; a
    sharded context; no residue"""
    _ffi.select("tuning")
    os.environ.pop("PVW_STAGE_BYTES", None)
    rng = random.Random(7)
    n, k, l, t, lb, pm, K = 40, 32, 8, 7, 52, SECP_N, 3
    moduli = M.bench_moduli(3)
    p, gpk, _ = system(moduli, n, k, l)
    assert p._lib.pvw_build_is_tuning() == 1
    D = 7
    secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(D, tag=3)
    coeffs = [unreduced(pm, rng, t)] + [[rng.getrandbits(256) for _ in range(t)] for _ in range(D - 1)]
    part = _params(n, k, l, moduli, (13, 31, 0, 32))
    for what, kw in (("drawn", dict(seeds=seeds)), ("explicit", dict(coeffs=coeffs))):
        want = P.shamir_shares_packed_wide(p, secrets, K, t, pm, host=True, **kw)
        item = (n + (t if "coeffs" in kw else 0) + K) * 32
        os.environ["PVW_STAGE_BYTES"] = str(3 * item + 4)          # pieces of 3, 3, 1 dealers
        try:
            got = P.shamir_shares_packed_wide(p, secrets, K, t, pm, **kw)
            sh = P.shamir_shares_packed_wide(part, secrets, K, t, pm, **kw)
        finally:
            os.environ.pop("PVW_STAGE_BYTES", None)
        assert np.array_equal(got, want), ("shares in pieces", what)
        assert np.array_equal(sh[:, 13:31], want[:, 13:31]) and not sh[:, :13].any() and not sh[:, 31:].any(), ("sharded shares in pieces", what)
        assert api._secret_residue(p)[0] == 0 and api._secret_residue(part)[0] == 0
    print("pieces shares ok", flush=True)
    D = 5
    nl = P.shamir_wide_limbs(pm, lb)
    V = D * nl
    item = nl * (k + n) * p.L * l * 8 + K * 32
    b = 2 * (2 * item) + 8                                          # half the budget holds 2 dealers: pieces of 2, 2, 1
    secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(V, tag=5)
    ref_p, ref_gpk, _ = system(moduli, n, k, l)
    cseed = lambda x: P.DeviceRandomness.call_seed(S, x)
    with P.DeviceRandomness(p, S, 1000) as st:
        for repr in (P.REPR_NTT, P.REPR_POWER):
            want = two_step(ref_p, ref_gpk, secrets, K, t, pm, seeds, lb, repr)
            c = st.counter()
            want_rs = two_step(ref_p, ref_gpk, secrets, K, t, pm, [cseed(c + v) for v in range(V)], lb, repr)
            os.environ["PVW_STAGE_BYTES"] = str(b)
            try:
                got = flat(P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, seeds=seeds, limb_bits=lb, out_repr=repr))
                got_rs = flat(P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, randomness=st, limb_bits=lb, out_repr=repr))
            finally:
                os.environ.pop("PVW_STAGE_BYTES", None)
            assert same(got, want), ("deal in pieces", repr)
            assert same(got_rs, want_rs) and st.counter() == c + V, ("rs deal in pieces", repr)
            assert api._secret_residue(p)[0] == 0
    print("pieces deal ok", flush=True)


def concurrent():
    """four threads on one context through the host-buffer forms, each with its own pack, degree and prime, three rounds each:
    every result equals the single-threaded reference computed beforehand"""
    rng = random.Random(8)
    n, k, l, lb = 40, 32, 8, 52
    moduli = M.bench_moduli(3)
    p, gpk, _ = system(moduli, n, k, l)
    ref_p, ref_gpk, _ = system(moduli, n, k, l)
    jobs = []
    for i, (K, t, pm, D) in enumerate(((1, 9, SECP_N, 2), (3, 7, P255, 1), (5, 0, P64, 3), (8, 30, SECP_N, 2))):
        nl = P.shamir_wide_limbs(pm, lb)
        secrets, seeds = packed_secrets(pm, rng, D, K), seeds_for(D * nl, tag=i)
        want_sh = P.shamir_shares_packed_wide(ref_p, secrets, K, t, pm, seeds=seeds[:D] if t else None, host=True)
        want_ct = two_step(ref_p, ref_gpk, secrets, K, t, pm, seeds, lb, P.REPR_NTT)
        jobs.append((K, t, pm, secrets, seeds, D, want_sh, want_ct))
    errors = []
    gate = threading.Barrier(len(jobs))

    def run(job):
        K, t, pm, secrets, seeds, D, want_sh, want_ct = job
        try:
            gate.wait()
            for _ in range(3):
                got = P.shamir_shares_packed_wide(p, secrets, K, t, pm, seeds=seeds[:D] if t else None)
                assert np.array_equal(got, want_sh), ("shares", K)
                cts = flat(P.deal_party_shares_packed_wide(secrets, K, t, pm, gpk, seeds=seeds, limb_bits=lb))
                assert same(cts, want_ct), ("deal", K)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(job,)) for job in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert api._secret_residue(p)[0] == 0
    print("concurrent ok", flush=True)


CASES = {f.__name__: f for f in (shares, deal, rs, loop, hygiene, pieces, concurrent)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_PACKED_WIDE_OK")

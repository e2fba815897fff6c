"""Shamir shares on the device: shamir_eval_kernel<false> against pvw_shamir_shares_host, the fused deal against
pvw_encrypt_multi of the host shares, the _rs forms and stream capture, the whole loop down to the reconstructed sum of the valid
dealers' secrets, and key hygiene.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir.py; prints SHAMIR_OK."""
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
from _util import EXAMPLE_MODULI, TEST_MODULI  # noqa: E402
from test_shamir_host import P31, P61, P62, next_prime, primes_for, secrets_for, seeds_for  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
S = bytes(range(101, 133))          # the randomness state's seed
U64 = (1 << 64) - 1


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def words(v):
    return np.array([int(x) & U64 for x in v], dtype=np.uint64)


def seed_bytes(seeds):
    return np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()


def _params(n, k=2, l=8, moduli=TEST_MODULI, shard=None):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if shard:
        b = b.set_shard(*shard)
    return b.build()


def device_shares(p, secrets, t, pm, seeds=None, coeffs=None, stream=None, fill=0):
    """pvw_shamir_shares_device on `stream`: the (D, n) buffer, pre-filled with `fill`"""
    D = len(secrets)
    out = torch.full((D, p.n), fill, dtype=torch.int64, device=DEV)
    d_se = dev(words(secrets))
    d_co = None if coeffs is None else dev(np.array(coeffs, dtype=np.uint64).reshape(D, -1))
    sd = None if seeds is None else seed_bytes(seeds)
    s = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    p._call("pvw_shamir_shares_device", ptr(d_se), D, t, pm, api._ptr(sd), ptr(d_co), ptr(out), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return u64(out)


def shares():
    """device shares == host shares: the grid of the host test (every p, degree, n, D of the contract), drawn and explicit
    coefficients, unreduced words, n not a multiple of 64, D beyond one launch (64 keys) and beyond one pass (128 dealers), the
    device-pointer form on a caller's stream and the host-buffer form; degrees that put a wave's term range on a chunk edge; a
    sharded context writes its own columns only"""
    rng = random.Random(1)
    s = torch.cuda.Stream(device=DEV)
    for n in (3, 64, 100, 1000):
        p = _params(n)
        mid = max(1, (n - 1) // 2)
        for D in (1, 5, 130):
            for pm in primes_for(n):
                for t in sorted({0, 1, 2, mid, n - 1}):
                    if t >= n:
                        continue
                    secrets, seeds = secrets_for(D, pm, rng), seeds_for(D, tag=t)
                    want = P.shamir_shares(p, secrets, t, pm, seeds=seeds, host=True)
                    got = device_shares(p, secrets, t, pm, seeds=seeds, stream=s)
                    assert np.array_equal(got, want), ("drawn", n, D, pm, t)
                    if t in (2, n - 1):
                        assert np.array_equal(P.shamir_shares(p, secrets, t, pm, seeds=seeds), want), ("host-buffer", n, D, pm, t)
                    if t and pm in (next_prime(n), P62):
                        coeffs = [[pm - 1] * t for _ in range(D)] if D != 5 else [[rng.getrandbits(64) for _ in range(t)] for _ in range(D)]
                        want = P.shamir_shares(p, secrets, t, pm, coeffs=coeffs, host=True)
                        assert np.array_equal(device_shares(p, secrets, t, pm, coeffs=coeffs, stream=s), want), ("explicit", n, D, pm, t)
                        if t == n - 1:
                            assert np.array_equal(P.shamir_shares(p, secrets, t, pm, coeffs=coeffs), want), ("explicit host-buffer", n, D, pm)
        print(f"shares n={n} ok", flush=True)
    # a wave's term range on a chunk edge (SH_JC = 64 terms per wave and chunk, Q = ceil(t / 4)): at t = 255 the last wave is one
    # term short of a full chunk, at 256 every wave holds exactly one, at 257 Q = 65 and wave 3 has no term in the second chunk
    n, D = 300, 5
    p = _params(n)
    for t in (255, 256, 257):
        for pm in (next_prime(n), P62):
            secrets, seeds = secrets_for(D, pm, rng), seeds_for(D, tag=t)
            coeffs = [[pm - 1] * t] + [[rng.getrandbits(64) for _ in range(t)] for _ in range(D - 1)]
            for what, kw in (("drawn", dict(seeds=seeds)), ("explicit", dict(coeffs=coeffs))):
                want = P.shamir_shares(p, secrets, t, pm, host=True, **kw)
                assert np.array_equal(device_shares(p, secrets, t, pm, stream=s, **kw), want), ("chunk edge", what, pm, t)
    print("shares chunk edges ok", flush=True)
    # sharded: columns [party_lo, party_hi) are written, the others keep what the buffer held
    n, D, t, pm = 200, 70, 77, P61
    lo, hi = 37, 171
    full, part = _params(n), _params(n, shard=(lo, hi, 0, 1))
    secrets, seeds = secrets_for(D, pm, rng), seeds_for(D)
    want = P.shamir_shares(full, secrets, t, pm, seeds=seeds, host=True)
    got = device_shares(part, secrets, t, pm, seeds=seeds, stream=s, fill=-7)
    marker = np.uint64(U64 - 6)
    assert np.array_equal(got[:, lo:hi], want[:, lo:hi]) and (got[:, :lo] == marker).all() and (got[:, hi:] == marker).all()
    hb = P.shamir_shares(part, secrets, t, pm, seeds=seeds)
    assert np.array_equal(hb[:, lo:hi], want[:, lo:hi]) and not hb[:, :lo].any() and not hb[:, hi:].any()
    print("shares shard ok", flush=True)


def system(moduli, n, k, l, shard=None, keys=False):
    p = _params(n, k, l, moduli, shard)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = None
    if keys:
        parties = [P.Party.new(i, p, SEED) for i in range(n)]
        gpk.generate_all_party_keys(parties, SEED)
    else:
        gpk.fill_uniform(SEED)
    return p, gpk, parties


def two_step(p, gpk, secrets, t, pm, seeds, repr):
    sh = P.shamir_shares(p, secrets, t, pm, seeds=seeds, host=True)
    return P.encrypt_many(sh.tolist(), gpk, seeds, repr)


def deal_device(p, secrets, t, pm, repr, stream, seeds=None, st=None):
    D = len(secrets)
    rA, rB = p.c1_hi - p.c1_lo, p.party_hi - p.party_lo
    c1 = torch.zeros((D, rA, p.L, p.l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((D, rB, p.L, p.l), dtype=torch.int64, device=DEV)
    d_se = dev(words(secrets))
    torch.cuda.synchronize()
    if st is None:
        p._call("pvw_deal_shares_device", ptr(d_se), D, t, pm, api._ptr(seed_bytes(seeds)), ptr(c1), ptr(c2), repr, C.c_void_p(stream.cuda_stream))
    else:
        p._call("pvw_deal_shares_rs_device", ptr(d_se), D, t, pm, st._h, ptr(c1), ptr(c2), repr, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(c1), u64(c2)


def same(cts, want):
    return all(np.array_equal(a.c1, b.c1) and np.array_equal(a.c2, b.c2) for a, b in zip(cts, want)) and len(cts) == len(want)


def deal():
    """pvw_deal_shares[_device] == pvw_encrypt_multi[_device] of the host shares under the same seeds, bit for bit: D = 2 (VALU)
    and 5, 64, 130 (matrix cores), NTT and power output, the 17-limb 61-bit chain and the 4 x 56-bit set (7-byte contraction),
    host-buffer and device-pointer forms, a sharded context"""
    rng = random.Random(2)
    s = torch.cuda.Stream(device=DEV)
    n, k, l = 40, 64, 8
    for name, moduli in (("17x61", M.bench_moduli(17)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, _ = system(moduli, n, k, l)
        for D in (2, 5, 64, 130):
            for repr, t, pm in ((P.REPR_NTT, n - 1, P61), (P.REPR_POWER, 7, P31)):
                secrets, seeds = secrets_for(D, pm, rng), seeds_for(D, tag=D)
                want = two_step(p, gpk, secrets, t, pm, seeds, repr)
                got = P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds, out_repr=repr)
                assert same(got, want), ("host-buffer", name, D, repr)
                g1, g2 = deal_device(p, secrets, t, pm, repr, s, seeds=seeds)
                for d in range(D):
                    assert np.array_equal(g1[d], want[d].c1) and np.array_equal(g2[d], want[d].c2), ("device", name, D, repr, d)
        print(f"deal {name} ok", flush=True)
    # sharded: ragged party and CRS-row ranges, both sides of the dispatch
    n, k = 70, 64
    shard = (13, 51, 16, 61)
    moduli = M.bench_moduli(3)
    full, gfull, _ = system(moduli, n, k, l)
    part, gpart, _ = system(moduli, n, k, l, shard)
    for D in (2, 9):
        secrets, seeds = secrets_for(D, P62, rng), seeds_for(D, tag=40 + D)
        want = two_step(full, gfull, secrets, 33, P62, seeds, P.REPR_NTT)
        g1, g2 = deal_device(part, secrets, 33, P62, P.REPR_NTT, s, seeds=seeds)
        for d in range(D):
            assert np.array_equal(g1[d], want[d].c1[16:61]) and np.array_equal(g2[d], want[d].c2[13:51]), ("shard device", D, d)
        got = P.deal_party_shares(secrets, 33, P62, gpart, seeds=seeds)
        for d in range(D):
            assert np.array_equal(got[d].c1[16:61], want[d].c1[16:61]) and np.array_equal(got[d].c2[13:51], want[d].c2[13:51]), ("shard host", D, d)
    print("deal shard ok", flush=True)


def rs():
    """the _rs forms with state (S, c) equal the seeded forms with seeds call_seed(S, c + d), the counter reads c + D afterwards
    (host-buffer and device-pointer, both sides of the dispatch, two passes); under stream capture without pvw_prepare the call is
    refused and the capture survives; captured after pvw_prepare(PVW_PREPARE_MFMA) and replayed twice, the replays give different
    ciphertexts that each decrypt to a valid sharing of the same secrets"""
    lib = _ffi.lib()
    rng = random.Random(3)
    n, k, l, t, pm = 24, 32, 8, 5, P61
    p, gpk, parties = system(M.bench_moduli(5), n, k, l, keys=True)
    s = torch.cuda.Stream(device=DEV)
    c = 77
    cseed = lambda x: P.DeviceRandomness.call_seed(S, x)
    with P.DeviceRandomness(p, S, c) as st:
        for D in (2, 5, 130):
            secrets = secrets_for(D, pm, rng)
            want = two_step(p, gpk, secrets, t, pm, [cseed(c + d) for d in range(D)], P.REPR_NTT)
            g1, g2 = deal_device(p, secrets, t, pm, P.REPR_NTT, s, st=st)
            for d in range(D):
                assert np.array_equal(g1[d], want[d].c1) and np.array_equal(g2[d], want[d].c2), ("rs device", D, d)
            c += D
            assert st.counter(s) == c, (D, st.counter(s))
            want = two_step(p, gpk, secrets, t, pm, [cseed(c + d) for d in range(D)], P.REPR_POWER)
            got = P.deal_party_shares(secrets, t, pm, gpk, randomness=st, out_repr=P.REPR_POWER)
            assert same(got, want), ("rs host", D)
            c += D
            assert st.counter() == c, D
        print("rs forms ok", flush=True)
        # The residue report covers every workspace of a context, and below 3 dealers pvw_encrypt_multi (the reference of the
        # comparison) leaves its r-hat vectors in one: in the capture part the context under test makes the deal calls only, and
        # a twin context with the same seeds (same CRS, same keys) computes the references and decrypts.
        ref_p, ref_gpk, ref_parties = system(M.bench_moduli(5), n, k, l, keys=True)
        for D in (2, 6):                                        # VALU path and matrix cores
            secrets = [rng.randrange(pm) for _ in range(D)]
            d_se = dev(words(secrets))
            c1 = torch.zeros((D, k, p.L, l), dtype=torch.int64, device=DEV)
            c2 = torch.zeros((D, n, p.L, l), dtype=torch.int64, device=DEV)
            enqueue = lambda cs: lib.pvw_deal_shares_rs_device(p._h, ptr(d_se), D, t, pm, st._h, ptr(c1), ptr(c2), P.REPR_NTT, cs)
            # not prepared: a stream the context has never seen
            s0 = torch.cuda.Stream(device=DEV)
            torch.cuda.synchronize()
            g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g0, stream=s0):
                rc = enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
                msg = _ffi.last_error(lib)
            torch.cuda.synchronize()
            assert rc == 1 and "pvw_prepare" in msg, (D, rc, msg)
            del g0
            assert st.counter(s) == c
            s1 = torch.cuda.Stream(device=DEV)
            p.prepare(P.PREPARE_MFMA, s1.cuda_stream)
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
                want = two_step(ref_p, ref_gpk, secrets, t, pm, [cseed(c + d) for d in range(D)], P.REPR_NTT)
                for d in range(D):
                    assert np.array_equal(g1[d], want[d].c1) and np.array_equal(g2[d], want[d].c2), ("replay", D, rep, d)
                c += D
                # every party decrypts its share of every dealer; any t + 1 of them give the dealer's secret back
                cts = [P.PvwCiphertext(g1[d], g2[d], ref_p, P.REPR_NTT) for d in range(D)]
                r = P.decrypt_many_checked(cts, [pt.secret_key for pt in ref_parties], 0, plain_modulus=pm)
                vals = np.asarray(r.values).reshape(n, D)
                for _ in range(3):
                    idx = rng.sample(range(n), t + 1)
                    assert P.shamir_reconstruct(idx, [[int(vals[i][d]) for i in idx] for d in range(D)], pm) == secrets, ("sharing", D, rep)
                seen.append((g1, g2))
            assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1]), D
            assert st.counter(s1) == c, D
            del g
        print("rs capture ok", flush=True)


def loop():
    """the loop closed: D dealers with p = 2^61 - 1 and a validity mask, enough valid dealers that the aggregates pass 2^64 (within
    sum_capacity()), aggregate_ciphertexts -> decrypt_all_party_sums(plain_modulus = p) -> shamir_reconstruct from three random
    subsets of t + 1 parties == the sum of the valid dealers' secrets mod p"""
    rng = random.Random(4)
    n, k, l, D, t, pm = 24, 32, 8, 40, 11, P61
    for name, moduli in (("5x61", M.bench_moduli(5)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, parties = system(moduli, n, k, l, keys=True)
        valid = np.arange(D) % 3 != 1
        count = int(valid.sum())
        assert 9 <= count <= p.sum_capacity(), (name, count, p.sum_capacity())
        secrets = [pm - 1 - rng.randrange(1 << 20) for _ in range(D)]
        seeds = seeds_for(D, tag=9)
        cts = P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds)
        sh = P.shamir_shares(p, secrets, t, pm, seeds=seeds, host=True)
        totals = [sum(int(sh[d][i]) for d in range(D) if valid[d]) for i in range(n)]
        assert max(totals) >= 1 << 64, name                    # the aggregates do pass 2^64
        agg = P.aggregate_ciphertexts(cts, valid)
        r = P.decrypt_all_party_sums([agg], parties, plain_modulus=pm)
        r2 = P.decrypt_all_party_sums(cts, parties, valid, plain_modulus=pm)
        got = [int(v) for v in r.values]
        assert got == [x % pm for x in totals] and got == [int(v) for v in r2.values], name
        want = sum(s for d, s in enumerate(secrets) if valid[d]) % pm
        for _ in range(3):
            idx = rng.sample(range(n), t + 1)
            assert P.shamir_reconstruct(idx, [got[i] for i in idx], pm) == want, (name, idx)
        print(f"loop {name} ok", flush=True)


def hygiene():
    """pvw_selftest_secret_residue reports zero after a host-buffer deal and after a device-pointer deal once its stream is drained
    (both sides of the dispatch), and after the host-buffer share call; the scanned regions are not empty"""
    rng = random.Random(5)
    n, k, l, t, pm = 40, 64, 8, 20, P61
    p, gpk, _ = system(M.bench_moduli(3), n, k, l)
    s = torch.cuda.Stream(device=DEV)
    for D in (2, 9, 130):
        secrets, seeds = secrets_for(D, pm, rng), seeds_for(D)
        P.deal_party_shares(secrets, t, pm, gpk, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= min(D, 128) * n, ("host-buffer", D, nz, scanned)
        deal_device(p, secrets, t, pm, P.REPR_NTT, s, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= min(D, 128) * n, ("device", D, nz, scanned)
        P.shamir_shares(p, secrets, t, pm, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= D * n, ("shares", D, nz, scanned)
    print("hygiene ok", flush=True)


def full():
    """config 3 (n = 4096), D = 64, degree 2047, p = 2^61 - 1: all device shares against pvw_shamir_shares_host"""
    rng = random.Random(6)
    n, D, t, pm = 4096, 64, 2047, P61
    p = _params(n, 256, 8, M.bench_moduli(17))
    secrets, seeds = secrets_for(D, pm, rng), seeds_for(D)
    want = P.shamir_shares(p, secrets, t, pm, seeds=seeds, host=True)
    got = device_shares(p, secrets, t, pm, seeds=seeds)
    assert np.array_equal(got, want)
    print("full ok", flush=True)


CASES = {f.__name__: f for f in (shares, deal, rs, loop, hygiene, full)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_OK")

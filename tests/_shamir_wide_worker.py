"""Shamir shares over a prime field of up to 256 bits on the device: shamir_eval_wide_kernel against
pvw_shamir_shares_wide_host, its Horner step against Python's integers, the fused deal against pvw_encrypt_multi of the host
shares' limb planes, the _rs forms and stream capture, the whole loop down to the reconstructed sum of the dealers' secrets, and
key hygiene.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_wide.py; prints SHAMIR_WIDE_OK."""
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
from test_shamir_wide_host import PRIMES, SECP_N, W256, ints, seeds_for  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
S = bytes(range(101, 133))          # the randomness state's seed
SHW_JC = 256                        # the kernel's staging chunk, in terms (degree + 1 of them)
FIRST, MIDDLE, LAST = PRIMES[0], PRIMES[len(PRIMES) // 2], PRIMES[-1]


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def seed_bytes(seeds):
    return np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()


def _params(n, k=2, l=8, moduli=TEST_MODULI, shard=None):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if shard:
        b = b.set_shard(*shard)
    return b.build()


def unreduced(p, rng, count):
    fixed = [W256, 0, p, p - 1, W256 - 1, 1 << 255]
    return [fixed[i] if i < len(fixed) else rng.getrandbits(256) for i in range(count)]


def device_shares(p, secrets, t, pm, seeds=None, coeffs=None, stream=None, fill=0):
    """pvw_shamir_shares_wide_device on `stream`: the (D, n, 4) buffer, pre-filled with `fill`"""
    D = len(secrets)
    out = torch.full((D, p.n, 4), fill, dtype=torch.int64, device=DEV)
    d_se = dev(api._wide(secrets))
    d_co = None if coeffs is None or t == 0 else dev(api._wide([v for row in coeffs for v in row]))
    sd = None if seeds is None else seed_bytes(seeds)
    s = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    p._call("pvw_shamir_shares_wide_device", ptr(d_se), D, t, api._ptr(api._wide_modulus(pm)), api._ptr(sd), ptr(d_co), ptr(out),
            C.c_void_p(s.cuda_stream))
    s.synchronize()
    return u64(out)


def shares():
    """device shares == host shares, bit for bit: n not a multiple of 64 or 256 and beyond one workgroup, D of 1, 5 and 27,
    degrees 0, 1, n - 1 and those that put degree + 1 on either side of the staging chunk, drawn and explicit coefficients,
    unreduced words, the first, middle and last prime of the list, the device-pointer and the host-buffer form; a sharded
    context writes its own columns only"""
    rng = random.Random(1)
    s = torch.cuda.Stream(device=DEV)
    for n in (3, 70, 300):
        p = _params(n)
        degrees = sorted({0, 1, n - 1} | ({SHW_JC - 2, SHW_JC - 1, SHW_JC, SHW_JC + 1} if n > SHW_JC + 1 else set()))
        for D in (1, 5, 27):
            for pm in (FIRST, MIDDLE, LAST):
                for t in degrees:
                    if D == 27 and t not in (1, n - 1):
                        continue
                    secrets, seeds = unreduced(pm, rng, D), seeds_for(D, tag=t)
                    want = P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds, host=True)
                    got = device_shares(p, secrets, t, pm, seeds=seeds, stream=s)
                    assert np.array_equal(got, want), ("drawn", n, D, pm, t)
                    if t in (1, n - 1):
                        assert np.array_equal(P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds), want), ("host-buffer", n, D, pm, t)
                    if t and D != 27:
                        coeffs = [unreduced(pm, rng, t)] + [[rng.getrandbits(256) for _ in range(t)] for _ in range(D - 1)]
                        want = P.shamir_shares_wide(p, secrets, t, pm, coeffs=coeffs, host=True)
                        assert np.array_equal(device_shares(p, secrets, t, pm, coeffs=coeffs, stream=s), want), ("explicit", n, D, pm, t)
                        if t == n - 1:
                            assert np.array_equal(P.shamir_shares_wide(p, secrets, t, pm, coeffs=coeffs), want), ("explicit host-buffer", n, D, pm)
        print(f"shares n={n} ok", flush=True)
    # more dealers than one launch carries keys for (64): the second launch starts at dealer 64 with its own keys
    n, D, t, pm = 70, 70, 5, MIDDLE
    p = _params(n)
    secrets, seeds = unreduced(pm, rng, D), seeds_for(D, tag=70)
    want = P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds, host=True)
    assert np.array_equal(device_shares(p, secrets, t, pm, seeds=seeds, stream=s), want), "two launches"
    assert np.array_equal(P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds), want), "two launches, host-buffer"
    print("shares two launches ok", flush=True)
    # sharded: columns [party_lo, party_hi) are written, the others keep what the buffer held
    n, D, t, pm = 300, 5, 77, SECP_N
    lo, hi = 37, 295
    full, part = _params(n), _params(n, shard=(lo, hi, 0, 1))
    secrets, seeds = unreduced(pm, rng, D), seeds_for(D)
    want = P.shamir_shares_wide(full, secrets, t, pm, seeds=seeds, host=True)
    got = device_shares(part, secrets, t, pm, seeds=seeds, stream=s, fill=-7)
    marker = np.uint64((1 << 64) - 7)
    assert np.array_equal(got[:, lo:hi], want[:, lo:hi]) and (got[:, :lo] == marker).all() and (got[:, hi:] == marker).all()
    hb = P.shamir_shares_wide(part, secrets, t, pm, seeds=seeds)
    assert np.array_equal(hb[:, lo:hi], want[:, lo:hi]) and not hb[:, :lo].any() and not hb[:, hi:].any()
    print("shares shard ok", flush=True)


def step():
    """pvw_selftest_shamir_wide_step == (acc x + add) mod p for every prime of the list on the edge operands of the CPU test,
    x = 2^32 - 1 included, and on random ones"""
    rng = random.Random(2)
    lib = _ffi.lib()
    p = _params(3)
    for pm in PRIMES:
        cases = [(a, x, b) for a in (0, pm - 1, rng.randrange(pm)) for b in (0, pm - 1, rng.randrange(pm))
                 for x in (1, 2, 1 << 16, (1 << 32) - 1, rng.getrandbits(32))]
        cases += [(rng.randrange(pm), rng.getrandbits(rng.randrange(1, 33)), rng.randrange(pm)) for _ in range(500)]
        acc, add = api._wide([c[0] for c in cases]), api._wide([c[2] for c in cases])
        x = np.array([c[1] for c in cases], dtype=np.uint64)
        out = np.zeros((len(cases), 4), dtype=np.uint64)
        api._check(lib.pvw_selftest_shamir_wide_step(p._h, api._ptr(api._wide_modulus(pm)), api._ptr(acc), api._ptr(x), api._ptr(add),
                                                     len(cases), api._ptr(out)), lib)
        assert ints(out) == [(a * xx + b) % pm for a, xx, b in cases], pm
    x = np.array([1 << 32], dtype=np.uint64)
    one = api._wide([1])
    assert lib.pvw_selftest_shamir_wide_step(p._h, api._ptr(api._wide_modulus(SECP_N)), api._ptr(one), api._ptr(x), api._ptr(one), 1,
                                             api._ptr(np.zeros((1, 4), dtype=np.uint64))) == 1
    print("step ok", flush=True)


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


def limb_planes(p, secrets, t, pm, seeds, limb_bits):
    """the scalars of the D * NL vectors: row d * NL + w is limb w of dealer d's host shares, drawn under seeds[d * NL]"""
    nl = P.shamir_wide_limbs(pm, limb_bits)
    sh = P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds[::nl], host=True)
    return np.concatenate([P.shamir_wide_to_limbs(sh[d], limb_bits, nl) for d in range(len(secrets))]), nl


def two_step(p, gpk, secrets, t, pm, seeds, limb_bits, repr):
    rows, _ = limb_planes(p, secrets, t, pm, seeds, limb_bits)
    return P.encrypt_many(rows.tolist(), gpk, seeds, repr)


def deal_device(p, secrets, t, pm, limb_bits, repr, stream, seeds=None, st=None):
    D = len(secrets)
    V = D * P.shamir_wide_limbs(pm, limb_bits)
    rA, rB = p.c1_hi - p.c1_lo, p.party_hi - p.party_lo
    c1 = torch.zeros((V, rA, p.L, p.l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((V, rB, p.L, p.l), dtype=torch.int64, device=DEV)
    d_se = dev(api._wide(secrets))
    pmw = api._ptr(api._wide_modulus(pm))
    torch.cuda.synchronize()
    if st is None:
        p._call("pvw_deal_shares_wide_device", ptr(d_se), D, t, pmw, limb_bits, api._ptr(seed_bytes(seeds)), ptr(c1), ptr(c2), repr,
                C.c_void_p(stream.cuda_stream))
    else:
        p._call("pvw_deal_shares_wide_rs_device", ptr(d_se), D, t, pmw, limb_bits, st._h, ptr(c1), ptr(c2), repr, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(c1), u64(c2)


def flat(cts):
    return [ct for dealer in cts for ct in dealer]


def same(cts, want):
    return all(np.array_equal(a.c1, b.c1) and np.array_equal(a.c2, b.c2) for a, b in zip(cts, want)) and len(cts) == len(want)


def deal():
    """pvw_deal_shares_wide[_device] == pvw_encrypt_multi of the host shares' limb planes under the same seeds, bit for bit:
    D * NL = 2 (VALU) and 5, 10, 70, 135 (matrix cores; 70 one-limb dealers are more than one launch carries keys for, 135 is more
    than one pass of 128, with dealer 25's limbs on both sides of the cut), NTT and power output, 52- and 62-bit limbs, the 17-limb 61-bit chain and the 4 x 56-bit set, host-buffer and
    device-pointer forms, a sharded context"""
    rng = random.Random(3)
    s = torch.cuda.Stream(device=DEV)
    n, k, l = 40, 64, 8
    for name, moduli in (("17x61", M.bench_moduli(17)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, _ = system(moduli, n, k, l)
        for D, pm, lb, repr, t in ((1, 2**89 - 1, 52, P.REPR_NTT, n - 1), (2, FIRST, 62, P.REPR_POWER, 7), (1, LAST, 52, P.REPR_POWER, 7),
                                   (2, SECP_N, 62, P.REPR_NTT, n - 1), (27, SECP_N, 52, P.REPR_NTT, 7), (70, FIRST, 62, P.REPR_NTT, 7)):
            if D >= 27 and name != "17x61":
                continue
            nl = P.shamir_wide_limbs(pm, lb)
            secrets, seeds = unreduced(pm, rng, D), seeds_for(D * nl, tag=D)
            want = two_step(p, gpk, secrets, t, pm, seeds, lb, repr)
            got = flat(P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds, limb_bits=lb, out_repr=repr))
            assert same(got, want), ("host-buffer", name, D, nl, repr)
            g1, g2 = deal_device(p, secrets, t, pm, lb, repr, s, seeds=seeds)
            for v in range(D * nl):
                assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("device", name, D, nl, repr, v)
        print(f"deal {name} ok", flush=True)
    # sharded: ragged party and CRS-row ranges, both sides of the dispatch
    n, k = 70, 64
    moduli = M.bench_moduli(3)
    full, gfull, _ = system(moduli, n, k, l)
    part, gpart, _ = system(moduli, n, k, l, (13, 51, 16, 61))
    for D, pm, lb in ((1, 2**89 - 1, 52), (2, SECP_N, 52)):
        nl = P.shamir_wide_limbs(pm, lb)
        secrets, seeds = unreduced(pm, rng, D), seeds_for(D * nl, tag=40 + D)
        want = two_step(full, gfull, secrets, 33, pm, seeds, lb, P.REPR_NTT)
        g1, g2 = deal_device(part, secrets, 33, pm, lb, P.REPR_NTT, s, seeds=seeds)
        for v in range(D * nl):
            assert np.array_equal(g1[v], want[v].c1[16:61]) and np.array_equal(g2[v], want[v].c2[13:51]), ("shard device", D, v)
        got = flat(P.deal_party_shares_wide(secrets, 33, pm, gpart, seeds=seeds, limb_bits=lb))
        for v in range(D * nl):
            assert np.array_equal(got[v].c1[16:61], want[v].c1[16:61]) and np.array_equal(got[v].c2[13:51], want[v].c2[13:51]), ("shard host", D, v)
    print("deal shard ok", flush=True)


def decrypt_limbs(cts, parties, nl, D):
    """every party's limb-wise sum over the dealers: [nl][n] words"""
    return [[int(v) for v in P.decrypt_all_party_sums([cts[d * nl + w] for d in range(D)], parties).values] for w in range(nl)]


def rs():
    """the _rs forms with state (S, c) equal the seeded forms with seeds call_seed(S, c + v), the counter reads c + D NL afterwards
    (host-buffer and device-pointer, both sides of the dispatch); under stream capture without pvw_prepare the call is refused
    and the capture survives; captured after pvw_prepare(PVW_PREPARE_MFMA) and replayed twice, the replays give different
    ciphertexts that each decrypt to a valid sharing of the same secrets"""
    lib = _ffi.lib()
    rng = random.Random(4)
    n, k, l, t, lb = 24, 32, 8, 5, 52
    p, gpk, parties = system(M.bench_moduli(5), n, k, l, keys=True)
    s = torch.cuda.Stream(device=DEV)
    c = 77
    cseed = lambda x: P.DeviceRandomness.call_seed(S, x)
    with P.DeviceRandomness(p, S, c) as st:
        for D, pm in ((1, 2**89 - 1), (3, SECP_N), (70, FIRST)):          # 70 one-limb dealers: two launches of the share kernel
            nl = P.shamir_wide_limbs(pm, lb)
            V = D * nl
            secrets = unreduced(pm, rng, D)
            want = two_step(p, gpk, secrets, t, pm, [cseed(c + v) for v in range(V)], lb, P.REPR_NTT)
            g1, g2 = deal_device(p, secrets, t, pm, lb, P.REPR_NTT, s, st=st)
            for v in range(V):
                assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("rs device", D, v)
            c += V
            assert st.counter(s) == c, (D, st.counter(s))
            want = two_step(p, gpk, secrets, t, pm, [cseed(c + v) for v in range(V)], lb, P.REPR_POWER)
            got = flat(P.deal_party_shares_wide(secrets, t, pm, gpk, randomness=st, limb_bits=lb, out_repr=P.REPR_POWER))
            assert same(got, want), ("rs host", D)
            c += V
            assert st.counter() == c, D
        print("rs forms ok", flush=True)
        # a twin context computes the references and decrypts (the residue report covers every workspace of a context)
        ref_p, ref_gpk, ref_parties = system(M.bench_moduli(5), n, k, l, keys=True)
        pmw = api._wide_modulus(SECP_N)
        for D, pm in ((1, 2**89 - 1), (2, SECP_N)):            # VALU path and matrix cores
            nl = P.shamir_wide_limbs(pm, lb)
            V = D * nl
            pmw = api._wide_modulus(pm)
            secrets = [rng.randrange(pm) for _ in range(D)]
            d_se = dev(api._wide(secrets))
            c1 = torch.zeros((V, k, p.L, l), dtype=torch.int64, device=DEV)
            c2 = torch.zeros((V, n, p.L, l), dtype=torch.int64, device=DEV)
            enqueue = lambda cs: lib.pvw_deal_shares_wide_rs_device(p._h, ptr(d_se), D, t, api._ptr(pmw), lb, st._h, ptr(c1), ptr(c2), P.REPR_NTT, cs)
            s0 = torch.cuda.Stream(device=DEV)                 # not prepared: a stream the context has never seen
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
                want = two_step(ref_p, ref_gpk, secrets, t, pm, [cseed(c + v) for v in range(V)], lb, P.REPR_NTT)
                for v in range(V):
                    assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("replay", D, rep, v)
                c += V
                # every party decrypts its limbs of every dealer; any t + 1 of the folded shares give the dealer's secret back
                cts = [P.PvwCiphertext(g1[v], g2[v], ref_p, P.REPR_NTT) for v in range(V)]
                for d in range(D):
                    sh = P.shamir_wide_from_limbs(decrypt_limbs(cts[d * nl:(d + 1) * nl], ref_parties, nl, 1), pm, lb)
                    idx = rng.sample(range(n), t + 1)
                    assert P.shamir_reconstruct_wide(idx, [sh[i] for i in idx], pm) == secrets[d], ("sharing", D, rep, d)
                seen.append((g1, g2))
            assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1]), D
            assert st.counter(s1) == c, D
            del g
        print("rs capture ok", flush=True)


def loop():
    """the loop closed over the secp256k1 order: five dealers deal, the ciphertexts are summed limb by limb
    (aggregate_ciphertexts), every party decrypts its limb sums (decrypt_all_party_sums), folds them back mod p
    (shamir_wide_from_limbs) and a random subset of t + 1 parties reconstructs the sum of the secrets"""
    rng = random.Random(5)
    n, k, l, D, t, pm, lb = 24, 32, 8, 5, 11, SECP_N, 52
    p, gpk, parties = system(M.bench_moduli(5), n, k, l, keys=True)
    nl = P.shamir_wide_limbs(pm, lb)
    secrets = [pm - 1 - rng.randrange(1 << 100) for _ in range(D)]
    cts = P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds_for(D * nl, tag=9), limb_bits=lb)
    sums = []
    for w in range(nl):
        agg = P.aggregate_ciphertexts([cts[d][w] for d in range(D)])
        sums.append([int(v) for v in P.decrypt_all_party_sums([agg], parties).values])
    assert max(max(row) for row in sums) >= 1 << lb                # the limb sums do leave the limb's width
    got = P.shamir_wide_from_limbs(sums, pm, lb)
    sh = ints(P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds_for(D * nl, tag=9)[::nl], host=True))
    assert got == [sum(sh[d][i] for d in range(D)) % pm for i in range(n)]
    for _ in range(3):
        idx = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct_wide(idx, [got[i] for i in idx], pm) == sum(secrets) % pm, idx
    print("loop ok", flush=True)


def hygiene():
    """pvw_selftest_secret_residue reports zero after a host-buffer deal and after a device-pointer deal once its stream is drained
    (both sides of the dispatch, more than one pass), and after the host-buffer share call; the scanned regions are not empty"""
    rng = random.Random(6)
    n, k, l, t, lb = 40, 64, 8, 20, 52
    p, gpk, _ = system(M.bench_moduli(3), n, k, l)
    s = torch.cuda.Stream(device=DEV)
    for D, pm in ((1, 2**89 - 1), (2, SECP_N), (27, SECP_N)):
        nl = P.shamir_wide_limbs(pm, lb)
        V = D * nl
        secrets, seeds = unreduced(pm, rng, D), seeds_for(V)
        P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds, limb_bits=lb)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= min(V, 128) * n, ("host-buffer", D, nz, scanned)
        deal_device(p, secrets, t, pm, lb, P.REPR_NTT, s, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= min(V, 128) * n, ("device", D, nz, scanned)
        P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds[:D])
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= D * n * 4, ("shares", D, nz, scanned)
    print("hygiene ok", flush=True)


def pieces():
    """the host-buffer forms staged in more than one piece (the measurement build's PVW_STAGE_BYTES): the shares at
    D = 7 in pieces of 3 dealers, drawn and explicit; the deal at D = 5 in pieces of 2 dealers (10 limb vectors each), seeded and
    from a randomness state, whose later pieces start from the counter the earlier ones left; a sharded context; no residue"""
    _ffi.select("tuning")
    os.environ.pop("PVW_STAGE_BYTES", None)
    rng = random.Random(7)
    n, k, l, t, lb, pm = 40, 32, 8, 7, 52, SECP_N
    moduli = M.bench_moduli(3)
    p, gpk, _ = system(moduli, n, k, l)
    assert p._lib.pvw_build_is_tuning() == 1
    D = 7
    secrets, seeds = unreduced(pm, rng, D), seeds_for(D, tag=3)
    coeffs = [unreduced(pm, rng, t)] + [[rng.getrandbits(256) for _ in range(t)] for _ in range(D - 1)]
    part = _params(n, k, l, moduli, (13, 31, 0, 32))
    for what, kw in (("drawn", dict(seeds=seeds)), ("explicit", dict(coeffs=coeffs))):
        want = P.shamir_shares_wide(p, secrets, t, pm, host=True, **kw)
        item = (n + (t if "coeffs" in kw else 0) + 1) * 32
        os.environ["PVW_STAGE_BYTES"] = str(3 * item + 4)          # pieces of 3, 3, 1 dealers
        try:
            got = P.shamir_shares_wide(p, secrets, t, pm, **kw)
            sh = P.shamir_shares_wide(part, secrets, t, pm, **kw)
        finally:
            os.environ.pop("PVW_STAGE_BYTES", None)
        assert np.array_equal(got, want), ("shares in pieces", what)
        assert np.array_equal(sh[:, 13:31], want[:, 13:31]) and not sh[:, :13].any() and not sh[:, 31:].any(), ("sharded shares in pieces", what)
        assert api._secret_residue(p)[0] == 0 and api._secret_residue(part)[0] == 0
    print("pieces shares ok", flush=True)
    D = 5
    nl = P.shamir_wide_limbs(pm, lb)
    V = D * nl
    item = nl * (k + n) * p.L * l * 8 + 32
    b = 2 * (2 * item) + 8                                          # half the budget holds 2 dealers: pieces of 2, 2, 1
    secrets, seeds = unreduced(pm, rng, D), seeds_for(V, tag=5)
    ref_p, ref_gpk, _ = system(moduli, n, k, l)                     # the references' r-hat stays out of the residue report
    cseed = lambda x: P.DeviceRandomness.call_seed(S, x)
    with P.DeviceRandomness(p, S, 1000) as st:
        for repr in (P.REPR_NTT, P.REPR_POWER):
            want = two_step(ref_p, ref_gpk, secrets, t, pm, seeds, lb, repr)
            c = st.counter()
            want_rs = two_step(ref_p, ref_gpk, secrets, t, pm, [cseed(c + v) for v in range(V)], lb, repr)
            os.environ["PVW_STAGE_BYTES"] = str(b)
            try:
                got = flat(P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds, limb_bits=lb, out_repr=repr))
                got_rs = flat(P.deal_party_shares_wide(secrets, t, pm, gpk, randomness=st, limb_bits=lb, out_repr=repr))
            finally:
                os.environ.pop("PVW_STAGE_BYTES", None)
            assert same(got, want), ("deal in pieces", repr)
            assert same(got_rs, want_rs) and st.counter() == c + V, ("rs deal in pieces", repr)
            assert api._secret_residue(p)[0] == 0
    print("pieces deal ok", flush=True)


CASES = {f.__name__: f for f in (shares, step, deal, rs, loop, hygiene, pieces)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_OK")

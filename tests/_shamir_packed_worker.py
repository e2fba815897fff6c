"""Packed Shamir sharing on the device: shamir_eval_kernel<true> and its weights against
pvw_shamir_shares_packed_host, the fused deal against pvw_encrypt_multi of the host shares, the _rs forms and stream capture, the
whole loop down to the corrected sums of the valid dealers' secrets, key hygiene, staged pieces and concurrent calls.
_shamir_worker imports torch FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_packed.py; prints SHAMIR_PACKED_OK."""
import ctypes as C
import os
import random
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from _shamir_worker import DEV, S, U64, _params, dev, ptr, same, seed_bytes, system, torch, u64  # noqa: E402
from _shamir_worker import device_shares as unpacked_device_shares  # noqa: E402
import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import EXAMPLE_MODULI  # noqa: E402
from test_shamir_host import P31, P61, P62, next_prime, seeds_for  # noqa: E402
from test_shamir_packed_host import first_prime_from, packed_secrets  # noqa: E402

MARK = np.uint64(U64 - 6)


def rows64(rows):
    return np.array([[int(v) & U64 for v in r] for r in rows], dtype=np.uint64)


def device_shares(p, secrets, t, pm, seeds=None, coeffs=None, stream=None):
    """pvw_shamir_shares_packed_device on `stream`: the (D, n) buffer, pre-filled with MARK"""
    se = rows64(secrets)
    D, K = se.shape
    out = torch.full((D, p.n), -7, dtype=torch.int64, device=DEV)
    d_se = dev(se)
    d_co = None if coeffs is None else dev(rows64(coeffs).reshape(D, -1))
    sd = None if seeds is None else seed_bytes(seeds)
    s = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    p._call("pvw_shamir_shares_packed_device", ptr(d_se), D, K, t, pm, api._ptr(sd), ptr(d_co), ptr(out), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return u64(out)


# (n, (party_lo, party_hi) of the sharded twin, [D], [(K, t)]): SH_JC = 64 terms per wave and chunk, 4 waves, Q = ceil((K + t) / 4)
SHAPES = [
    (3, (1, 3), [1, 5], [(1, 2), (2, 1), (3, 0)]),                       # fewer terms than waves; t = 0 draws nothing
    (64, (5, 50), [5], [(1, 63), (64, 0), (32, 32), (33, 31), (5, 2)]),  # the secret/random boundary on a wave edge and inside a range
    (100, (37, 99), [130], [(3, 50), (50, 50)]),                         # D beyond PVW_MAX_PROLOGUE_KEYS; n not a multiple of 64
    (300, (70, 267), [5], [(130, 140), (256, 1), (1, 299)]),             # Q > 64: two chunks per wave; boundary on a chunk edge
    (1000, (130, 901), [1], [(500, 500)]),                               # four chunks
]


def shares():
    """device shares == host shares at every shape, with drawn and with explicit coefficients, on a whole context and on a sharded
    one whose party_lo is no multiple of 64 (its other columns keep what the buffer held), device-pointer and host-buffer forms;
    pack = 1 equals pvw_shamir_shares_device, and on the chunk edges of its term axis both equal pvw_shamir_shares_host"""
    rng = random.Random(1)
    s = torch.cuda.Stream(device=DEV)
    for n, (lo, hi), Ds, kts in SHAPES:
        full, part = _params(n), _params(n, shard=(lo, hi, 0, 1))
        for D in Ds:
            for K, t in kts:
                for pm in (first_prime_from(n + K), P61):
                    secrets, seeds = packed_secrets(D, K, pm, rng), seeds_for(D, tag=K + t)
                    coeffs = [[rng.getrandbits(64) for _ in range(t)] for _ in range(D)]
                    if t:
                        coeffs[0] = [pm - 1] * t
                    forms = [("drawn", dict(seeds=seeds if t else None))] + ([("explicit", dict(coeffs=coeffs))] if t else [])
                    for what, kw in forms:
                        want = P.shamir_shares_packed(full, secrets, t, pm, host=True, **kw)
                        tag = (what, n, D, K, t, pm)
                        assert np.array_equal(device_shares(full, secrets, t, pm, stream=s, **kw), want), tag
                        got = device_shares(part, secrets, t, pm, stream=s, **kw)
                        assert np.array_equal(got[:, lo:hi], want[:, lo:hi]), ("shard",) + tag
                        assert (got[:, :lo] == MARK).all() and (got[:, hi:] == MARK).all(), ("shard columns",) + tag
                        if pm == P61:
                            assert np.array_equal(P.shamir_shares_packed(full, secrets, t, pm, **kw), want), ("host-buffer",) + tag
                            hb = P.shamir_shares_packed(part, secrets, t, pm, **kw)
                            assert np.array_equal(hb[:, lo:hi], want[:, lo:hi]) and not hb[:, :lo].any() and not hb[:, hi:].any(), tag
        print(f"shares n={n} ok", flush=True)
    # pack = 1: the packed instantiation gives the words of the unpacked one
    n, D, pm = 100, 70, P62
    p = _params(n)
    for t in (0, 1, 50, 99):
        secrets, seeds = [rng.getrandbits(64) for _ in range(D)], seeds_for(D, tag=t)
        old = P.shamir_shares(p, secrets, t, pm, seeds=seeds)
        assert np.array_equal(device_shares(p, [[x] for x in secrets], t, pm, seeds=seeds if t else None, stream=s), old), ("pack 1", t)
    # ... and on the chunk edges of the unpacked term axis (_shamir_worker.shares), both equal to the host restatement
    n, D = 300, 5
    p = _params(n)
    for t in (255, 256, 257):
        for pm in (next_prime(n), P62):
            secrets, seeds = [rng.getrandbits(64) for _ in range(D)], seeds_for(D, tag=t)
            coeffs = [[pm - 1] * t] + [[rng.getrandbits(64) for _ in range(t)] for _ in range(D - 1)]
            for what, kw in (("drawn", dict(seeds=seeds)), ("explicit", dict(coeffs=coeffs))):
                want = P.shamir_shares(p, secrets, t, pm, host=True, **kw)
                assert np.array_equal(unpacked_device_shares(p, secrets, t, pm, stream=s, **kw), want), ("chunk edge unpacked", what, pm, t)
                assert np.array_equal(device_shares(p, [[x] for x in secrets], t, pm, stream=s, **kw), want), ("chunk edge pack 1", what, pm, t)
    print("shares pack=1 ok", flush=True)


def two_step(p, gpk, secrets, t, pm, seeds, repr):
    sh = P.shamir_shares_packed(p, secrets, t, pm, seeds=seeds, host=True)
    return P.encrypt_many(sh.tolist(), gpk, seeds, repr)


def deal_device(p, secrets, t, pm, repr, stream, seeds=None, st=None):
    se = rows64(secrets)
    D, K = se.shape
    rA, rB = p.c1_hi - p.c1_lo, p.party_hi - p.party_lo
    c1 = torch.zeros((D, rA, p.L, p.l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((D, rB, p.L, p.l), dtype=torch.int64, device=DEV)
    d_se = dev(se)
    torch.cuda.synchronize()
    cs = C.c_void_p(stream.cuda_stream)
    if st is None:
        p._call("pvw_deal_shares_packed_device", ptr(d_se), D, K, t, pm, api._ptr(seed_bytes(seeds)), ptr(c1), ptr(c2), repr, cs)
    else:
        p._call("pvw_deal_shares_packed_rs_device", ptr(d_se), D, K, t, pm, st._h, ptr(c1), ptr(c2), repr, cs)
    stream.synchronize()
    return u64(c1), u64(c2)


def deal():
    """pvw_deal_shares_packed[_device] == pvw_encrypt_multi of the host shares under the same seeds, bit for bit: D = 2 (VALU) and
    5 (matrix cores), NTT and power output, the 17-limb 61-bit chain and the 4 x 56-bit set, host-buffer and device-pointer forms,
    at n = 64, (K, t) = (8, 20); a sharded context; pack = 1 equals pvw_deal_shares*; on a context with keys every packed refusal
    is reached through the four deal forms and writes nothing"""
    rng = random.Random(2)
    s = torch.cuda.Stream(device=DEV)
    n, k, l, K, t = 64, 32, 8, 8, 20
    for name, moduli in (("17x61", M.bench_moduli(17)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, _ = system(moduli, n, k, l)
        for D in (2, 5):
            for repr, pm in ((P.REPR_NTT, P61), (P.REPR_POWER, P31)):
                secrets, seeds = packed_secrets(D, K, pm, rng), seeds_for(D, tag=D)
                want = two_step(p, gpk, secrets, t, pm, seeds, repr)
                got = P.deal_party_shares_packed(secrets, t, pm, gpk, seeds=seeds, out_repr=repr)
                assert same(got, want), ("host-buffer", name, D, repr)
                g1, g2 = deal_device(p, secrets, t, pm, repr, s, seeds=seeds)
                for d in range(D):
                    assert np.array_equal(g1[d], want[d].c1) and np.array_equal(g2[d], want[d].c2), ("device", name, D, repr, d)
            # pack = 1: the ciphertexts of pvw_deal_shares*
            one = [rng.getrandbits(64) for _ in range(D)]
            seeds = seeds_for(D, tag=50 + D)
            old = P.deal_party_shares(one, t, P61, gpk, seeds=seeds)
            assert same(P.deal_party_shares_packed([[x] for x in one], t, P61, gpk, seeds=seeds), old), ("pack 1 host", name, D)
            g1, g2 = deal_device(p, [[x] for x in one], t, P61, P.REPR_NTT, s, seeds=seeds)
            for d in range(D):
                assert np.array_equal(g1[d], old[d].c1) and np.array_equal(g2[d], old[d].c2), ("pack 1 device", name, D, d)
        print(f"deal {name} ok", flush=True)
    # on a context with keys the packed refusals are reached through the deal entry points themselves, in every form
    se, sd = np.arange(3 * K, dtype=np.uint64), np.zeros(3 * 32, dtype=np.uint8)
    h1, h2 = np.zeros((3, k, p.L, l), np.uint64), np.zeros((3, n, p.L, l), np.uint64)
    d_se, d1, d2 = dev(se), dev(h1), dev(h2)
    with P.DeviceRandomness(p, S, 5) as st:
        for pack, deg, pm in ((0, 2, P61), (K, n - K + 1, P61), (K, 2, n + K - 1), (K, 2, 561), (K, 2, 1 << 62)):
            calls = (("pvw_deal_shares_packed", (api._ptr(se), 3, pack, deg, pm, api._ptr(sd), api._ptr(h1), api._ptr(h2), P.REPR_NTT)),
                     ("pvw_deal_shares_packed_rs", (api._ptr(se), 3, pack, deg, pm, st._h, api._ptr(h1), api._ptr(h2), P.REPR_NTT)),
                     ("pvw_deal_shares_packed_device", (ptr(d_se), 3, pack, deg, pm, api._ptr(sd), ptr(d1), ptr(d2), P.REPR_NTT, None)),
                     ("pvw_deal_shares_packed_rs_device", (ptr(d_se), 3, pack, deg, pm, st._h, ptr(d1), ptr(d2), P.REPR_NTT, None)))
            for fn, args in calls:
                try:
                    p._call(fn, *args)
                    raise AssertionError((fn, pack, deg, pm, "accepted"))
                except P.PvwError as e:
                    assert e.code == 1, (fn, pack, deg, pm, e)
        assert st.counter() == 5 and not h1.any() and not h2.any() and not u64(d1).any() and not u64(d2).any()
    print("deal refusals ok", flush=True)
    # sharded: ragged party and CRS-row ranges, both sides of the dispatch
    n = 70
    lo, hi, a, b = 13, 51, 5, 29
    moduli = M.bench_moduli(3)
    full, gfull, _ = system(moduli, n, k, l)
    part, gpart, _ = system(moduli, n, k, l, (lo, hi, a, b))
    for D in (2, 9):
        secrets, seeds = packed_secrets(D, K, P62, rng), seeds_for(D, tag=40 + D)
        want = two_step(full, gfull, secrets, 33, P62, seeds, P.REPR_NTT)
        g1, g2 = deal_device(part, secrets, 33, P62, P.REPR_NTT, s, seeds=seeds)
        for d in range(D):
            assert np.array_equal(g1[d], want[d].c1[a:b]) and np.array_equal(g2[d], want[d].c2[lo:hi]), ("shard device", D, d)
        got = P.deal_party_shares_packed(secrets, 33, P62, gpart, seeds=seeds)
        for d in range(D):
            assert np.array_equal(got[d].c1[a:b], want[d].c1[a:b]) and np.array_equal(got[d].c2[lo:hi], want[d].c2[lo:hi]), ("shard host", D, d)
    print("deal shard ok", flush=True)


def rs():
    """the _rs forms with state (S, c) equal the seeded forms with seeds call_seed(S, c + d) and leave c + D (host-buffer and
    device-pointer, both sides of the dispatch); under stream capture a call is refused, and the capture survives, until the
    stream has its share scratch AND weights of that size; one capture replayed twice deals two different sharings of the same
    secrets, and both reconstruct"""
    lib = _ffi.lib()
    rng = random.Random(3)
    n, k, l, K, t, pm = 24, 32, 8, 4, 5, P61
    p, gpk, parties = system(M.bench_moduli(5), n, k, l, keys=True)
    s = torch.cuda.Stream(device=DEV)
    c = 77
    cseed = lambda x: P.DeviceRandomness.call_seed(S, x)
    with P.DeviceRandomness(p, S, c) as st:
        for D in (2, 5):
            secrets = packed_secrets(D, K, pm, rng)
            want = two_step(p, gpk, secrets, t, pm, [cseed(c + d) for d in range(D)], P.REPR_NTT)
            g1, g2 = deal_device(p, secrets, t, pm, P.REPR_NTT, s, st=st)
            for d in range(D):
                assert np.array_equal(g1[d], want[d].c1) and np.array_equal(g2[d], want[d].c2), ("rs device", D, d)
            c += D
            assert st.counter(s) == c, (D, st.counter(s))
            want = two_step(p, gpk, secrets, t, pm, [cseed(c + d) for d in range(D)], P.REPR_POWER)
            got = P.deal_party_shares_packed(secrets, t, pm, gpk, randomness=st, out_repr=P.REPR_POWER)
            assert same(got, want), ("rs host", D)
            c += D
            assert st.counter() == c, D
        print("rs forms ok", flush=True)
        # the context under test makes deal calls only (pvw_encrypt_multi below 3 dealers leaves r-hat in a workspace, which the
        # residue report would find): a twin with the same seeds computes the references and decrypts
        ref_p, ref_gpk, ref_parties = system(M.bench_moduli(5), n, k, l, keys=True)
        for D in (2, 6):                                        # VALU path and matrix cores
            secrets = [[rng.randrange(pm) for _ in range(K)] for _ in range(D)]
            d_se = dev(rows64(secrets))
            c1 = torch.zeros((D, k, p.L, l), dtype=torch.int64, device=DEV)
            c2 = torch.zeros((D, n, p.L, l), dtype=torch.int64, device=DEV)
            # D dealers whatever the pack: c1 and c2 hold D ciphertexts, d_se at least D * pack words
            enqueue = lambda cs, pack=K: lib.pvw_deal_shares_packed_rs_device(p._h, ptr(d_se), D, pack, t, pm, st._h, ptr(c1), ptr(c2),
                                                                              P.REPR_NTT, cs)

            def refused(stream, why):
                torch.cuda.synchronize()
                g0 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g0, stream=stream):
                    rc = enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    msg = _ffi.last_error(lib)
                torch.cuda.synchronize()
                assert rc == 1 and "pvw_prepare" in msg, (why, D, rc, msg)
                del g0
                assert st.counter(s) == c, why
            refused(torch.cuda.Stream(device=DEV), "a stream the context has never seen")
            s1 = torch.cuda.Stream(device=DEV)
            p.prepare(P.PREPARE_MFMA, s1.cuda_stream)
            refused(s1, "prepared, but no weights sized")
            api._check(enqueue(C.c_void_p(s1.cuda_stream), pack=2), lib)   # pack 2 outside capture: too few words for pack 4
            s1.synchronize()
            c += D
            refused(s1, "weights sized for a smaller pack")
            api._check(enqueue(C.c_void_p(s1.cuda_stream)), lib)           # the same call outside capture sizes the weights
            s1.synchronize()
            c += D
            assert st.counter(s1) == c
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
                # every party decrypts its share of every dealer; any t + K of them give the dealer's secrets back
                cts = [P.PvwCiphertext(g1[d], g2[d], ref_p, P.REPR_NTT) for d in range(D)]
                r = P.decrypt_many_checked(cts, [pt.secret_key for pt in ref_parties], 0, plain_modulus=pm)
                vals = np.asarray(r.values).reshape(n, D)
                for _ in range(2):
                    idx = rng.sample(range(n), t + K)
                    assert P.shamir_reconstruct_packed(idx, [[int(vals[i][d]) for i in idx] for d in range(D)], pm, K) == secrets, (D, rep)
                seen.append((g1, g2))
            assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1]), D
            assert st.counter(s1) == c, D
            del g
        print("rs capture ok", flush=True)


def loop():
    """the loop closed: D dealers of K secrets each with p = 2^61 - 1 and a validity mask, deal packed -> aggregate_ciphertexts ->
    decrypt_all_party_sums(plain_modulus = p) -> shamir_reconstruct_packed_corrected on the device == sum_d s_{d,j} over the valid
    dealers for every j; once more with two parties' sums corrupted, which the decode names"""
    rng = random.Random(4)
    n, k, l, D, K, t, pm = 24, 32, 8, 12, 4, 5, P61
    for name, moduli in (("5x61", M.bench_moduli(5)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, parties = system(moduli, n, k, l, keys=True)
        valid = np.arange(D) % 3 != 1
        assert int(valid.sum()) <= p.sum_capacity(), (name, p.sum_capacity())
        secrets = [[pm - 1 - rng.randrange(1 << 20) for _ in range(K)] for _ in range(D)]
        cts = P.deal_party_shares_packed(secrets, t, pm, gpk, seeds=seeds_for(D, tag=9))
        agg = P.aggregate_ciphertexts(cts, valid)
        r = P.decrypt_all_party_sums([agg], parties, plain_modulus=pm)
        got = [int(v) for v in r.values]
        want = [sum(s[j] for d, s in enumerate(secrets) if valid[d]) % pm for j in range(K)]
        idx = list(range(n))
        back, nerr, col_err, _ = P.shamir_reconstruct_packed_corrected(p, idx, [got], t, pm, K)
        assert back == [want] and nerr.tolist() == [0] and not col_err.any(), name
        for _ in range(2):
            sub = rng.sample(range(n), t + K)
            assert P.shamir_reconstruct_packed(sub, [[got[i] for i in sub]], pm, K) == [want], (name, sub)
        got[3] = (got[3] + 1) % pm
        got[17] = (got[17] + pm - 5) % pm
        back, nerr, col_err, mask = P.shamir_reconstruct_packed_corrected(p, idx, [got], t, pm, K)
        assert back == [want] and nerr.tolist() == [2], (name, back, nerr)
        assert [c for c in range(n) if col_err[c]] == [3, 17] and int(mask[0][0]) == (1 << 3) | (1 << 17), name
        # pack = 1 on the device: an ordinary sharing through the packed mirror is shamir_reconstruct_corrected
        one = [pm - 1 - rng.randrange(1 << 20) for _ in range(3)]
        sh1 = P.shamir_shares(p, one, t, pm, seeds=seeds_for(3, tag=1)).tolist()
        for row in sh1:
            row[rng.randrange(n)] ^= 1
        back, nerr, col_err, mask = P.shamir_reconstruct_packed_corrected(p, idx, sh1, t, pm, 1)
        ref = P.shamir_reconstruct_corrected(p, idx, sh1, t, pm)
        assert back == [[v] for v in one] and [r[0] for r in back] == ref[0] and nerr.tolist() == [1, 1, 1], (name, back, nerr)
        assert np.array_equal(col_err, ref[2]) and np.array_equal(mask, ref[3]), name
        print(f"loop {name} ok", flush=True)


def hygiene():
    """pvw_selftest_secret_residue reports zero after a host-buffer packed deal and after a device-pointer one once its stream is
    drained (below and above the matrix-core threshold), and after the host-buffer share call; the scanned regions are not empty"""
    rng = random.Random(5)
    n, k, l, K, t, pm = 40, 32, 8, 6, 20, P61
    p, gpk, _ = system(M.bench_moduli(3), n, k, l)
    s = torch.cuda.Stream(device=DEV)
    for D in (2, 9):
        secrets, seeds = packed_secrets(D, K, pm, rng), seeds_for(D)
        P.deal_party_shares_packed(secrets, t, pm, gpk, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= D * n, ("host-buffer", D, nz, scanned)
        deal_device(p, secrets, t, pm, P.REPR_NTT, s, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= D * n, ("device", D, nz, scanned)
        P.shamir_shares_packed(p, secrets, t, pm, seeds=seeds)
        nz, scanned = api._secret_residue(p)
        assert nz == 0 and scanned >= D * (n + K), ("shares", D, nz, scanned)
    print("hygiene ok", flush=True)


def staged():
    """the tuning build with a small PVW_STAGE_BYTES: pvw_shamir_shares_packed at D = 7 in pieces [3, 3, 1] and
    pvw_deal_shares_packed at D = 9 in passes [4, 4, 1] (seeded and _rs) give the words of the one-piece calls and of the host
    restatement, and leave nothing behind.  The library's piece arithmetic is restated here so no call quietly runs in one piece"""
    _ffi.select("tuning")
    os.environ.pop("PVW_STAGE_BYTES", None)
    rng = random.Random(6)
    n, k, l, K, t, pm = 40, 32, 8, 6, 7, P61
    p, gpk, _ = system(M.bench_moduli(3), n, k, l)
    assert p._lib.pvw_build_is_tuning() == 1
    ref_p, ref_gpk, _ = system(M.bench_moduli(3), n, k, l)           # makes the pvw_encrypt_multi references (see rs())

    def budget(b):
        os.environ.pop("PVW_STAGE_BYTES", None)
        if b is not None:
            os.environ["PVW_STAGE_BYTES"] = str(b)
    cut = lambda D, per: [min(per, D - d0) for d0 in range(0, D, per)]
    D = 7
    secrets, seeds = packed_secrets(D, K, pm, rng), seeds_for(D)
    coeffs = [[rng.getrandbits(64) for _ in range(t)] for _ in range(D)]
    for what, kw, extra in (("drawn", dict(seeds=seeds), 0), ("explicit", dict(coeffs=coeffs), t)):
        item = (n + extra + K) * 8
        b = 3 * item + 4
        assert cut(D, min(max(b // item, 1), D)) == [3, 3, 1] and (1 << 30) // item >= D
        want = P.shamir_shares_packed(p, secrets, t, pm, host=True, **kw)
        for bb in (None, b):
            budget(bb)
            got = P.shamir_shares_packed(p, secrets, t, pm, **kw)
            budget(None)
            assert np.array_equal(got, want), ("shares", what, bb)
            assert api._secret_residue(p)[0] == 0, ("shares residue", what, bb)
    print("staged shares: pieces [3, 3, 1] ok", flush=True)
    D = 9
    secrets, seeds = packed_secrets(D, K, pm, rng), seeds_for(D, tag=3)
    item = (k + n) * p.L * l * 8 + K * 8
    b = 8 * item
    per = lambda bb: min(max((bb // 2) // item, 4) & ~3, D)
    assert cut(D, per(b)) == [4, 4, 1] and cut(D, per(1 << 30)) == [D]
    c0 = 500
    rs_seeds = [P.DeviceRandomness.call_seed(S, c0 + d) for d in range(D)]
    for repr in (P.REPR_NTT, P.REPR_POWER):
        want = two_step(ref_p, ref_gpk, secrets, t, pm, seeds, repr)
        want_rs = two_step(ref_p, ref_gpk, secrets, t, pm, rs_seeds, repr)
        for bb in (None, b):
            budget(bb)
            got = P.deal_party_shares_packed(secrets, t, pm, gpk, seeds=seeds, out_repr=repr)
            budget(None)
            assert same(got, want), ("deal", repr, bb)
            assert api._secret_residue(p)[0] == 0, ("deal residue", repr, bb)
            with P.DeviceRandomness(p, S, c0) as st:
                budget(bb)
                got = P.deal_party_shares_packed(secrets, t, pm, gpk, randomness=st, out_repr=repr)
                budget(None)
                assert st.counter() == c0 + D
            assert same(got, want_rs), ("deal rs", repr, bb)
            assert api._secret_residue(p)[0] == 0, ("deal rs residue", repr, bb)
    print("staged deal: passes [4, 4, 1] ok", flush=True)


def concurrent():
    """two threads on one context, each making host-buffer packed calls (a deal on either side of the dispatch and the share call)
    of its own inputs, several rounds behind a barrier: every result is the serial one"""
    rng = random.Random(7)
    n, k, l, K, t, pm = 40, 32, 8, 6, 20, P61
    p, gpk, _ = system(M.bench_moduli(3), n, k, l)
    jobs = []
    for i, D in enumerate((2, 9)):
        secrets, seeds = packed_secrets(D, K, pm, rng), seeds_for(D, tag=70 + i)
        jobs.append((secrets, seeds, two_step(p, gpk, secrets, t, pm, seeds, P.REPR_NTT),
                     P.shamir_shares_packed(p, secrets, t, pm, seeds=seeds, host=True)))
    rounds, errors = 4, []
    barrier = threading.Barrier(2)

    def run(i):
        secrets, seeds, want_ct, want_sh = jobs[i]
        try:
            for r in range(rounds):
                barrier.wait(timeout=60)
                if not same(P.deal_party_shares_packed(secrets, t, pm, gpk, seeds=seeds), want_ct):
                    errors.append((i, r, "deal"))
                if not np.array_equal(P.shamir_shares_packed(p, secrets, t, pm, seeds=seeds), want_sh):
                    errors.append((i, r, "shares"))
        except Exception as e:                                   # a broken barrier in the other thread must not hide this one
            errors.append((i, repr(e)))
            barrier.abort()
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errors and not any(th.is_alive() for th in threads), errors
    print("concurrent ok", flush=True)


CASES = {f.__name__: f for f in (shares, deal, rs, loop, hygiene, staged, concurrent)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_PACKED_OK")

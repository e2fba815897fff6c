"""Many weighted sums of the same dealers' ciphertexts on the device against pvw_ct_lincomb_many_host, the
single-row calls of DESIGN 8.12, the dealt Shamir shares and the packed sharing's secrets.  torch is imported FIRST so both
libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_ct_lincomb_many.py; prints CT_LINCOMB_MANY_OK."""
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
from test_ct_sum_host import GEOMETRIES, _params, _words  # noqa: E402
from test_ct_lincomb_host import I64_MAX, I64_MIN, PLAIN  # noqa: E402
from test_ct_lincomb_many_host import COMBOS, DEALERS, weight_rows  # noqa: E402
from _ct_lincomb_worker import budget, cur, dev, fills, ptr, system, u64, u8  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2B]) * 32
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)


def host_many(p, c1s, c2s, rows, valid, lo, hi):
    """pvw_ct_lincomb_many_host, the reference: (c1 [R][k], c2 [R][hi - lo], counts [R])"""
    R = len(rows)
    c1, c2 = np.zeros((R, p.k, p.L, p.l), np.uint64), np.zeros((R, hi - lo, p.L, p.l), np.uint64)
    cnt = np.zeros(R, np.uint32)
    w = np.ascontiguousarray(rows, dtype=np.int64)
    p._call("pvw_ct_lincomb_many_host", api._ptr(c1s), api._ptr(c2s), len(c1s), api._ptr(u8(valid)), api._ptr(w), R, lo, hi, api._ptr(c1),
            api._ptr(c2), api._ptr(cnt))
    return c1, c2, cnt.tolist()


def hostbuf_many(p, c1s, c2s, rows, valid, lo, hi):
    """pvw_ct_lincomb_many (host buffers)"""
    R = len(rows)
    c1, c2 = np.full((R, p.k, p.L, p.l), MARK), np.full((R, hi - lo, p.L, p.l), MARK)
    cnt = np.full(R, 77, np.uint32)
    w = np.ascontiguousarray(rows, dtype=np.int64)
    p._call("pvw_ct_lincomb_many", api._ptr(c1s), api._ptr(c2s), len(c1s), api._ptr(u8(valid)), api._ptr(w), R, lo, hi, api._ptr(c1),
            api._ptr(c2), api._ptr(cnt))
    return c1, c2, cnt.tolist()


def device_many(p, d_c1s, d_c2s, D, rows, valid, lo, hi, stream, name="pvw_ct_lincomb_many_device"):
    """pvw_ct_lincomb_many_device on `stream`, straight into marked buffers of exactly the result's size"""
    R = len(rows)
    c1 = torch.full((R, p.k, p.L, p.l), -1, dtype=torch.int64, device=DEV)
    c2 = torch.full((R, hi - lo, p.L, p.l), -1, dtype=torch.int64, device=DEV)
    cnt = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    v = None if valid is None else dev(u8(valid))
    w = dev(np.ascontiguousarray(rows, dtype=np.int64))
    torch.cuda.synchronize()
    if name == "pvw_ct_lincomb_many_device":
        p._call(name, ptr(d_c1s), ptr(d_c2s), D, ptr(v), ptr(w), R, lo, hi, ptr(c1), ptr(c2), ptr(cnt), C.c_void_p(stream.cuda_stream))
    else:                                                                # the single-row call of DESIGN 8.12
        p._call(name, ptr(d_c1s), ptr(d_c2s), D, ptr(v), ptr(w), lo, hi, ptr(c1), ptr(c2), ptr(cnt), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(c1), u64(c2), cnt.cpu().tolist()


def combos():
    """R x D of the host test on a caller's own stream with a row range inside [0, n): the shipped library, and the tuning build
    in the split forms PVW_SUM_SPLIT 1 / 3 / 64 with every instantiated row tile (PVW_SUM_RT 2 / 4 / 8); device form everywhere,
    host-buffer form in the shipped library, against pvw_ct_lincomb_many_host bit for bit, counts included; R = 1 against
    pvw_ct_lincomb_device; one shape that is unsplit by itself."""
    s = torch.cuda.Stream(device=DEV)
    forms = [("default", 0, 0)]
    if os.path.exists(_ffi.LIB_TUNING_PATH):
        forms += [("tuning", 1, 2), ("tuning", 3, 4), ("tuning", 64, 8), ("tuning", 64, 2), ("tuning", 3, 8)]
    for which, split, rt in forms:
        _ffi.select(which)
        os.environ["PVW_SUM_SPLIT"], os.environ["PVW_SUM_RT"] = str(split), str(rt)
        calls = 0
        for geom, (n, k, l, moduli) in enumerate(GEOMETRIES):
            if which == "tuning" and (geom + split + rt) % 2:            # every tuning form on half of the geometries
                continue
            p = _params(n, k, l, moduli)
            ranges = [(0, n), (1, n - 1), (n - 1, n), (1, 2)]
            for D in DEALERS:
                rng = np.random.default_rng(77 * geom + D)
                masks = [None, np.arange(D) % 2 == 0, np.arange(D) == D // 2]
                c1s, c2s = _words(rng, p, D, k, "any"), _words(rng, p, D, n, "any")
                for step, R in enumerate(COMBOS):
                    valid = masks[(step + geom) % 3]
                    wkind = ("ones", "uniform", "extreme")[(step + D) % 3]
                    lo, hi = ranges[(step + D) % 4]
                    h1, h2 = c1s.copy(), c2s.copy()
                    if valid is not None:                                # never read: the words of a masked-out dealer do not matter
                        h1[~valid], h2[~valid] = np.uint64((1 << 64) - 1), np.uint64((1 << 64) - 1)
                    rows = weight_rows(rng, moduli, R, D, wkind)
                    what = (which, split, rt, geom, D, R, wkind, lo, hi)
                    on = [int(np.count_nonzero((rows[r] != 0) & (True if valid is None else valid))) for r in range(R)]
                    g1, g2, cnt = device_many(p, dev(h1), dev(h2), D, rows, valid, lo, hi, s)
                    calls += 1
                    assert cnt == on, what
                    if any(on):
                        w1, w2, wc = host_many(p, h1, h2, rows, valid, lo, hi)
                        assert wc == on and np.array_equal(g1, w1) and np.array_equal(g2, w2), what
                    for r in range(R):
                        if on[r] == 0:                                   # nobody takes part: zeros, in every form
                            assert not g1[r].any() and not g2[r].any(), (what, r)
                    if R == 1:
                        o1, o2, oc = device_many(p, dev(h1), dev(h2), D, rows, valid, lo, hi, s, "pvw_ct_lincomb_device")
                        assert np.array_equal(g1, o1) and np.array_equal(g2, o2) and oc == cnt, what
                    if which == "default" and any(on) and (step + D) % 2 == 0:
                        b1, b2, bc = hostbuf_many(p, h1, h2, rows, valid, lo, hi)
                        assert np.array_equal(b1, w1) and np.array_equal(b2, w2) and bc == on, what
        print(f"combos {which} split={split} rt={rt} ok ({calls} device calls)", flush=True)
    os.environ.pop("PVW_SUM_SPLIT")
    os.environ.pop("PVW_SUM_RT")
    _ffi.select("default")
    # 520 workgroups of items: the unsplit form by the shape alone (config-3 geometry, rows 0..1700 of an n = 2048 context)
    n, k, l, D, R, hi = 2048, 256, 8, 9, 5, 1700
    p = _params(n, k, l, M.bench_moduli(17))
    assert ((k + hi) * p.L * l // 2 + 255) // 256 >= 512
    g = torch.Generator(device=DEV)
    g.manual_seed(D + n)
    d1 = torch.empty((D, k, p.L, l), dtype=torch.int64, device=DEV).random_(generator=g)
    d2 = torch.empty((D, n, p.L, l), dtype=torch.int64, device=DEV).random_(generator=g)
    for t in (d1, d2):                                                   # random_ leaves bit 63 clear
        t.bitwise_xor_(t.bitwise_left_shift(13))
    valid = np.arange(D) != 4
    rows = weight_rows(np.random.default_rng(9), M.bench_moduli(17), R, D, "uniform")
    w1, w2, wc = host_many(p, u64(d1), u64(d2), rows, valid, 0, hi)
    g1, g2, cnt = device_many(p, d1, d2, D, rows, valid, 0, hi, s)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and cnt == wc and cnt[R // 2] == 0
    print("unsplit by itself ok", flush=True)


# ---- the packed handover -----------------------------------------------------------------------------------------------------
class PackedHandover:
    """The recipe of DESIGN 8.15 / INTEGRATION: an old PACKED sharing F (K = 3 secrets, degree t + K - 1 = 4, made with
    shamir_shares_packed) whose holders d re-deal y_d = F(d + 1) with fresh polynomials of degree 2 (deal_party_shares); `masked`
    old holders are left out; the weight rows are shamir_packed_handover_weights over the valid old indices, 0 elsewhere.
    want[j][m] = sum_d lambda_{d,m} f_d(j + 1) mod p from pvw_shamir_shares_host; exact[j][m] the same sum as an integer."""
    K, T, DEGREE = 3, 2, 2

    def __init__(self, n, D, masked, k=16, l=8, tag=0):
        self.p, self.gpk, self.parties = system(M.bench_moduli(17), n, k, l)
        rnd = random.Random(100 * n + D + tag)
        self.secrets = [rnd.randrange(PLAIN) for _ in range(self.K)]
        old = _params(D, 2, 8)                                            # the old committee: D holders
        y = [int(x) for x in P.shamir_shares_packed(old, [self.secrets], self.T, PLAIN, [bytes([tag + 1]) * 32], host=True)[0]]
        seeds = [api._dealer_seed(SEED, 60 + tag + d) for d in range(D)]
        self.cts = P.deal_party_shares(y, self.DEGREE, PLAIN, self.gpk, seeds)
        self.shares = P.shamir_shares(self.p, y, self.DEGREE, PLAIN, seeds, host=True)          # [D][n]
        self.D, self.n = D, n
        self.c1s, self.c2s = np.stack([c.c1 for c in self.cts]), np.stack([c.c2 for c in self.cts])
        self.use(masked)

    def use(self, masked):
        D = self.D
        self.valid = np.array([d not in masked for d in range(D)], np.uint8)
        on = [d for d in range(D) if self.valid[d]]
        assert len(on) >= self.T + self.K
        self.rows = np.zeros((self.K, D), np.int64)
        self.rows[:, on] = P.shamir_packed_handover_weights(on, PLAIN, self.K)
        assert all(self.p.lincomb_fits(self.rows[m], self.valid) for m in range(self.K))
        self.exact = [[sum(int(self.rows[m][d]) * int(self.shares[d][j]) for d in on) for m in range(self.K)] for j in range(self.n)]
        self.want = [[x % PLAIN for x in row] for row in self.exact]
        return self


def report(r):
    return r.residues.tolist(), r.noise.tolist(), r.status.tolist()


def handover():
    """the packed handover on both sides of the 22-party dispatch: column m of the one call is sum_d lambda_{d,m} shares_d[j] mod p
    at every party, any three rows of it reconstruct secret m, each column equals the R = 1 call; POWER-basis input, wide words, a
    sub-range of parties, the device-pointer form; no key material left behind"""
    for n, D, masked in ((24, 9, (1, 6)), (6, 6, (3,))):
        h = PackedHandover(n, D, masked)
        p, parties, K = h.p, h.parties, h.K
        r = P.decrypt_all_party_combinations_many(h.cts, h.rows, parties, h.valid, plain_modulus=PLAIN)
        assert r.values.shape == (n, K) and r.values.tolist() == h.want, n
        assert r.valid.all() and r.bound >= 1 << 64, n
        assert api._secret_residue(p)[0] == 0
        rnd = random.Random(n)
        for m in range(K):
            for _ in range(4):
                who = rnd.sample(range(n), h.DEGREE + 1)
                assert P.shamir_reconstruct(who, [[h.want[j][m] for j in who]], PLAIN)[0] == h.secrets[m], (n, m, who)
            one = P.decrypt_all_party_combinations(h.cts, h.rows[m], parties, h.valid, plain_modulus=PLAIN)
            assert (r.residues[:, m].tolist(), r.noise[:, m].tolist(), r.status[:, m].tolist()) == report(one), (n, m)
        # the [P][R] report feeds the checked reconstruction in place: secret m from column m with strides (1, R)
        got, bad, _ = P.shamir_reconstruct_checked(p, list(range(n)), r.residues, h.DEGREE, PLAIN, layout="party_major")
        assert [int(x) for x in got] == h.secrets and not np.asarray(bad).any(), n
        # a sub-range of parties, POWER-basis input, wide words
        lo, cnt = 1, 4
        pw = [P.PvwCiphertext(p.ntt_inverse(c.c1), p.ntt_inverse(c.c2), p, P.REPR_POWER) for c in h.cts]
        rw = P.decrypt_all_party_combinations_many(pw, h.rows, parties[lo:lo + cnt], h.valid, plain_modulus=PLAIN, wide=True)
        assert [[int(x) for x in row] for row in rw.values] == h.exact[lo:lo + cnt] and rw.residues.tolist() == h.want[lo:lo + cnt], n
        assert rw.negative.tolist() == [[x < 0 for x in row] for row in h.exact[lo:lo + cnt]] and not rw.truncated.any(), n
        for m in range(K):
            one = P.decrypt_all_party_combinations(pw, h.rows[m], parties[lo:lo + cnt], h.valid, plain_modulus=PLAIN, wide=True)
            assert (rw.residues[:, m].tolist(), rw.noise[:, m].tolist(), rw.status[:, m].tolist()) == report(one), (n, m)
            assert [int(x) for x in rw.values[:, m]] == [int(x) for x in one.values], (n, m)
        assert api._secret_residue(p)[0] == 0
        # device pointers, both representations, with an extra all-zero row and a duplicate of row 0 (R = 5)
        W = (p.q_total().bit_length() + 63) // 64
        rows5 = np.concatenate([h.rows, np.zeros((1, D), np.int64), h.rows[:1]])
        R = len(rows5)
        sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
        dv, dw = dev(h.valid), dev(rows5)
        for rep_, cts in ((P.REPR_NTT, h.cts), (P.REPR_POWER, pw)):
            c1, c2 = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2 for c in cts]))
            out, nz = torch.full((n, R), -1, dtype=torch.int64, device=DEV), torch.full((n, R), -1, dtype=torch.int64, device=DEV)
            st, dc = torch.full((n, R), -1, dtype=torch.int32, device=DEV), torch.full((R,), -1, dtype=torch.int32, device=DEV)
            wide = torch.full((n, R, W), -1, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            p._call("pvw_decrypt_all_lincomb_many_plain_device", 0, n, ptr(sk), ptr(c1), ptr(c2), D, ptr(dv), ptr(dw), R, rep_, ptr(out),
                    ptr(nz), ptr(st), ptr(dc), PLAIN, W, ptr(wide), cur())
            torch.cuda.synchronize()
            assert dc.cpu().tolist() == [D - len(masked)] * K + [0, D - len(masked)], (n, rep_)
            o = u64(out)
            assert o[:, :K].tolist() == h.want and not o[:, K].any() and o[:, K + 1].tolist() == [row[0] for row in h.want], (n, rep_)
            assert not u64(nz)[:, K].any() and not u64(wide)[:, K].any(), (n, rep_)                # the zero ciphertext: 0, no noise
            neg = (st.cpu().numpy() & api.DEC_NEGATIVE) != 0
            for j in range(n):
                for m in range(K):
                    mag = sum(int(x) << (64 * i) for i, x in enumerate(u64(wide)[j, m]))
                    assert (-mag if neg[j, m] else mag) == h.exact[j][m], (n, rep_, j, m)
            assert np.array_equal(u64(nz)[:, :K], r.noise) and np.array_equal(u64(nz)[:, K + 1], r.noise[:, 0]), (n, rep_)
            assert api._secret_residue(p)[0] == 0
        # a masked-out dealer is not read even where its weights are not 0
        rows2 = h.rows.copy()
        rows2[:, masked[0]] = 12345
        r2 = P.decrypt_all_party_combinations_many(h.cts, rows2, parties, h.valid, plain_modulus=PLAIN)
        assert r2.values.tolist() == h.want, n
        print(f"handover n={n} ok", flush=True)


def hygiene():
    """after each decrypting form -- host buffers and device pointers, both representations, both sides of the dispatch, R cut
    into several groups (tuning build) -- pvw_selftest_secret_residue finds nothing; the grouped call equals the ungrouped one"""
    for which in ("default", "tuning"):
        if which == "tuning" and not os.path.exists(_ffi.LIB_TUNING_PATH):
            continue
        _ffi.select(which)
        for n, D, masked in ((24, 9, (1, 6)), (6, 6, (3,))):
            h = PackedHandover(n, D, masked, tag=3)
            p, parties = h.p, h.parties
            rows = np.concatenate([h.rows, h.rows[::-1], h.rows[:1]])                            # R = 7
            ref = P.decrypt_all_party_combinations_many(h.cts, rows, parties, h.valid, plain_modulus=PLAIN)
            assert api._secret_residue(p)[0] == 0
            assert ref.values[:, :3].tolist() == h.want and ref.values[:, 6].tolist() == [row[0] for row in h.want]
            if which == "tuning":                                        # groups of 3, 3, 1 combinations: one more pass over the dealers each
                with budget(3 * (p.k + n) * p.L * p.l * 8 + 64):
                    cut = P.decrypt_all_party_combinations_many(h.cts, rows, parties, h.valid, plain_modulus=PLAIN)
                assert report(cut) == report(ref), n
                assert api._secret_residue(p)[0] == 0
            pw = [P.PvwCiphertext(p.ntt_inverse(c.c1), p.ntt_inverse(c.c2), p, P.REPR_POWER) for c in h.cts]
            rp = P.decrypt_all_party_combinations_many(pw, rows, parties[1:5], h.valid, plain_modulus=PLAIN, wide=True)
            assert rp.residues.tolist() == ref.residues[1:5].tolist()
            assert api._secret_residue(p)[0] == 0
            P.combine_ciphertexts_many(h.cts, rows, h.valid)
            assert api._secret_residue(p)[0] == 0
        print(f"hygiene {which} ok", flush=True)
    _ffi.select("default")


def pieces():
    """the tuning build with PVW_STAGE_BYTES so small that pvw_ct_lincomb_many and pvw_decrypt_all_lincomb_many_plain take three
    and four staged pieces at D = 13, R = 5 (the accumulate path, every piece with its [R][per] weights), where one dealer takes
    part in one row only and one valid dealer in none: bit-equal to one piece and to pvw_ct_lincomb_many_host"""
    _ffi.select("tuning")
    n, D, R = 8, 13, 5
    p, gpk, parties = system(M.bench_moduli(17), n, 16, 8)
    Pw = p.L * p.l
    rng = np.random.default_rng(5)
    valid = np.array([d not in (2, 5, 6, 11) for d in range(D)], np.uint8)
    rows = rng.integers(I64_MIN, I64_MAX, (R, D), dtype=np.int64, endpoint=True)
    rows[:, 7] = 0                                                       # valid, weight 0 in every row: never staged
    rows[:, 9] = 0
    rows[3, 9] = -3                                                      # takes part in row 3 only
    rows[1, :] = 0                                                       # and a row nobody takes part in
    part = (valid != 0) & (rows != 0).any(axis=0)
    nv = int(part.sum())
    assert nv == 8 and part[9] and not part[7]
    c1s, c2s = _words(rng, p, D, p.k, "any"), _words(rng, p, D, n, "any")
    w1, w2, wc = host_many(p, c1s, c2s, rows, valid, 1, n)
    assert wc[1] == 0 and wc[3] == 8 and wc[0] == 7
    for per in (3, 2):
        item = (p.k + n - 1) * Pw * 8
        b = per * item + item // 2
        f = fills(part, per)
        assert len(f) == (3 if per == 3 else 4) and max(f) == per, f
        for bb in (None, b):
            with budget(bb):
                g1, g2, cnt = hostbuf_many(p, c1s, c2s, rows, valid, 1, n)
            assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and cnt == wc, ("ct_lincomb_many", per, bb)
        print(f"pieces ct_lincomb_many: {f}", flush=True)
    # the decrypt: small weights over dealt shares, so that every row decodes; the same participation pattern
    secrets = [int(x) for x in rng.integers(0, 1 << 40, D)]
    seeds = [api._dealer_seed(SEED, 90 + d) for d in range(D)]
    cts = P.deal_party_shares(secrets, 2, PLAIN, gpk, seeds)
    shares = P.shamir_shares(p, secrets, 2, PLAIN, seeds, host=True)
    small = rng.integers(-9, 10, (R, D), dtype=np.int64)
    small[small == 0] = 4
    small[rows == 0] = 0
    want = [[sum(int(small[r][d]) * int(shares[d][j]) for d in range(D) if valid[d]) % PLAIN for r in range(R)] for j in range(n)]
    for lo, cnt in ((0, n), (2, 3)):
        item = (p.k + cnt) * Pw * 8
        got = []
        for bb in (None, 3 * item + item // 2):
            with budget(bb):
                r = P.decrypt_all_party_combinations_many(cts, small, parties[lo:lo + cnt], valid, plain_modulus=PLAIN)
            got.append(report(r))
            assert r.valid.all() and api._secret_residue(p)[0] == 0
        assert got[0] == got[1] and got[0][0] == want[lo:lo + cnt], ("all parties", lo, cnt)
        print(f"pieces decrypt_all_lincomb_many_plain [{lo}, {lo + cnt}) ok", flush=True)
    _ffi.select("default")


def capture():
    """pvw_ct_lincomb_many_device captured after pvw_prepare(PVW_PREPARE_SUM) replays with changed weights and mask; the
    decrypt-all form is refused under capture on a stream nothing has sized, with nothing enqueued (the capture survives, its
    graph is empty of our work), and accepted after a sizing call outside capture, replaying like the eager call"""
    lib = _ffi.lib()
    n, D = 24, 9
    h = PackedHandover(n, D, (1, 6), tag=5)
    p, parties, K = h.p, h.parties, h.K
    R = K + 2
    c1, c2 = dev(h.c1s), dev(h.c2s)
    sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
    mask = dev(h.valid)
    weights = dev(np.concatenate([h.rows, h.rows[:2]]))

    def fresh():
        return {"c1": torch.full((R, p.k, p.L, p.l), -1, dtype=torch.int64, device=DEV), "c2": torch.full((R, n - 2, p.L, p.l), -1, dtype=torch.int64, device=DEV),
                "cnt": torch.full((R,), -1, dtype=torch.int32, device=DEV), "out": torch.full((n, R), -1, dtype=torch.int64, device=DEV),
                "nz": torch.full((n, R), -1, dtype=torch.int64, device=DEV), "st": torch.full((n, R), -1, dtype=torch.int32, device=DEV)}

    def comb(o, cs):
        rc = lib.pvw_ct_lincomb_many_device(p._h, ptr(c1), ptr(c2), D, ptr(mask), ptr(weights), R, 1, n - 1, ptr(o["c1"]), ptr(o["c2"]),
                                            ptr(o["cnt"]), cs)
        return rc, _ffi.last_error(lib)

    def dec(o, cs):
        rc = lib.pvw_decrypt_all_lincomb_many_plain_device(p._h, 0, n, ptr(sk), ptr(c1), ptr(c2), D, ptr(mask), ptr(weights), R, P.REPR_NTT,
                                                           ptr(o["out"]), ptr(o["nz"]), ptr(o["st"]), ptr(o["cnt"]), PLAIN, 0, None, cs)
        return rc, _ffi.last_error(lib)

    def same(a, b, keys):
        return all(torch.equal(a[k_], b[k_]) for k_ in keys)

    def settings():
        for rep, masked in enumerate(((1, 6), (0, 2, 3), ())):
            h.use(masked)
            rows = np.concatenate([h.rows, h.rows[:2]])
            if rep == 2:
                rows[1, :] = 0
                rows[4, 3] = I64_MIN
            mask.copy_(torch.from_numpy(h.valid))
            weights.copy_(torch.from_numpy(rows))
            torch.cuda.synchronize()
            yield rep, rows

    s = torch.cuda.Stream(device=DEV)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    torch.cuda.synchronize()
    # the decrypt-all form on this stream: PVW_PREPARE_SUM does not size its scratch
    captured, eager = fresh(), fresh()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s):
        rc, msg = dec(captured, cur())
    torch.cuda.synchronize()
    assert rc == 1 and "outside capture first" in msg, (rc, msg)
    g0.replay()                                                          # nothing of the refused call was enqueued
    torch.cuda.synchronize()
    assert same(captured, fresh(), ("out", "nz", "st", "cnt"))
    del g0
    # the combination: PVW_PREPARE_SUM suffices
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, msg = comb(captured, cur())
    assert rc == 0, msg
    for rep, rows in settings():
        g.replay()
        torch.cuda.synchronize()
        rc, msg = comb(eager, cur())
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert same(captured, eager, ("c1", "c2", "cnt")), rep
        w1, w2, wc = host_many(p, h.c1s, h.c2s, rows, h.valid, 1, n - 1)
        assert np.array_equal(u64(captured["c1"]), w1) and np.array_equal(u64(captured["c2"]), w2) and captured["cnt"].cpu().tolist() == wc, rep
    del g
    # a sizing call outside capture (the same party range, as many combinations), then the capture is accepted
    with torch.cuda.stream(s):
        rc, msg = dec(eager, cur())
    assert rc == 0, msg
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, msg = dec(captured, cur())
    assert rc == 0, msg
    for rep, rows in settings():
        g.replay()
        torch.cuda.synchronize()
        rc, msg = dec(eager, cur())
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert same(captured, eager, ("out", "nz", "st", "cnt")), rep
        if rep < 2:
            assert u64(captured["out"])[:, :K].tolist() == h.want, rep
    del g
    assert api._secret_residue(p)[0] == 0
    print("capture ok", flush=True)


def threads():
    """two threads on one context call pvw_ct_lincomb_many (R = 5 and R = 1), pvw_ct_lincomb_many_host and
    pvw_decrypt_all_lincomb_many_plain next to each other, round after round: every result is the serial twin's"""
    n, D = 6, 6
    h = PackedHandover(n, D, (3,), tag=7)
    p, parties = h.p, h.parties
    rng = np.random.default_rng(8)
    rows = rng.integers(I64_MIN, I64_MAX, (5, D), dtype=np.int64, endpoint=True)
    rows[2, :] = 0
    rows[:, 1] = 0
    c1s, c2s = _words(rng, p, D, p.k, "any"), _words(rng, p, D, n, "any")
    flat = lambda t: tuple(x.tobytes() if isinstance(x, np.ndarray) else tuple(x) for x in t)

    def job_comb():
        return flat(hostbuf_many(p, c1s, c2s, rows, h.valid, 1, n))

    def job_one():
        return flat(hostbuf_many(p, c1s, c2s, rows[:1], h.valid, 0, n))

    def job_host():
        return flat(host_many(p, c1s, c2s, rows, h.valid, 1, n))

    def job_all():
        return report(P.decrypt_all_party_combinations_many(h.cts, h.rows, parties, h.valid, plain_modulus=PLAIN))

    plans = [[job_comb, job_all, job_host, job_one, job_all], [job_all, job_comb, job_comb, job_all, job_one]]
    serial = [[job() for job in plan] for plan in plans]
    assert serial[0][0] == serial[0][2] and serial[0][1][0] == h.want
    rounds = 5
    barrier = threading.Barrier(2)
    got, errors = [[], []], []

    def work(t):
        try:
            for _ in range(rounds):
                for job in plans[t]:
                    barrier.wait(timeout=60)
                    got[t].append(job())
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))
            barrier.abort()

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for t in range(2):
        assert got[t] == serial[t] * rounds, ("thread", t)
    assert api._secret_residue(p)[0] == 0
    print("threads ok", flush=True)


CASES = {f.__name__: f for f in (combos, pieces, handover, hygiene, capture, threads)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("CT_LINCOMB_MANY_OK")

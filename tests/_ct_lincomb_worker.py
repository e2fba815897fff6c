"""Weighted sums of dealers' ciphertexts on the device against pvw_ct_lincomb_host, the dealt Shamir shares and
the host decodes.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_ct_lincomb.py; prints CT_LINCOMB_OK."""
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
from test_ct_lincomb_host import I64_MAX, I64_MIN, PLAIN, _weight_sets  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def u8(valid):
    return None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)


def host_lincomb(p, c1s, c2s, weights, valid, lo, hi):
    c1, c2 = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((hi - lo, p.L, p.l), np.uint64)
    w = np.ascontiguousarray(weights, dtype=np.int64)
    p._call("pvw_ct_lincomb_host", api._ptr(c1s), api._ptr(c2s), len(c1s), api._ptr(u8(valid)), api._ptr(w), lo, hi, api._ptr(c1),
            api._ptr(c2), None)
    return c1, c2


def hostbuf_lincomb(p, c1s, c2s, weights, valid, lo, hi):
    """pvw_ct_lincomb (host buffers): (c1, c2, count)"""
    c1, c2 = np.full((p.k, p.L, p.l), MARK), np.full((hi - lo, p.L, p.l), MARK)
    cnt = C.c_uint32(77)
    w = np.ascontiguousarray(weights, dtype=np.int64)
    p._call("pvw_ct_lincomb", api._ptr(c1s), api._ptr(c2s), len(c1s), api._ptr(u8(valid)), api._ptr(w), lo, hi, api._ptr(c1), api._ptr(c2),
            C.byref(cnt))
    return c1, c2, cnt.value


class DeviceOut:
    """the outputs of pvw_ct_lincomb_device, allocated once a geometry and marked before every call"""

    def __init__(self, p):
        self.c1 = torch.empty((p.k, p.L, p.l), dtype=torch.int64, device=DEV)
        self.c2 = torch.empty((p.n, p.L, p.l), dtype=torch.int64, device=DEV)
        self.cnt = torch.empty((1,), dtype=torch.int32, device=DEV)


def device_lincomb(p, o, d_c1s, d_c2s, D, weights, valid, lo, hi, stream):
    """pvw_ct_lincomb_device on `stream`: (c1, c2, count)"""
    o.c1.fill_(-1), o.c2.fill_(-1), o.cnt.fill_(-1)
    v = None if valid is None else dev(u8(valid))
    w = dev(np.ascontiguousarray(weights, dtype=np.int64))
    torch.cuda.synchronize()
    p._call("pvw_ct_lincomb_device", ptr(d_c1s), ptr(d_c2s), D, ptr(v), ptr(w), lo, hi, ptr(o.c1), ptr(o.c2), ptr(o.cnt),
            C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(o.c1), u64(o.c2)[:hi - lo], int(o.cnt.item())


def device_sum(p, o, d_c1s, d_c2s, D, valid, lo, hi, stream):
    """pvw_ct_sum_device on `stream`, the call the combination with every weight 1 is bit-equal to: (c1, c2, count)"""
    o.c1.fill_(-1), o.c2.fill_(-1), o.cnt.fill_(-1)
    v = None if valid is None else dev(u8(valid))
    torch.cuda.synchronize()
    p._call("pvw_ct_sum_device", ptr(d_c1s), ptr(d_c2s), D, ptr(v), lo, hi, ptr(o.c1), ptr(o.c2), ptr(o.cnt), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(o.c1), u64(o.c2)[:hi - lo], int(o.cnt.item())


def combos():
    """The host-test matrix on a caller's own stream, in the shipped library and in every kernel form of the tuning build
    (PVW_SUM_SPLIT 1 / 3 / 64): every geometry (l = 8 .. 64), D in {1, 2, 7, 130} with reduced / any / extreme words and, at
    the group and chunk edges of the dealer walk, D in {8, 9, 63, 64, 65} with any words; masks (all, alternating, one dealer,
    none); weights all 1 (and then bit-equal to pvw_ct_sum_device as well), uniform int64, the extremes, a set with zeros, all
    zero; the rotations of the extremes in the shipped library.  Device form (every library form) and host-buffer form (shipped
    library, any and extreme words) against pvw_ct_lincomb_host, bit for bit."""
    s = torch.cuda.Stream(device=DEV)
    inside_a_wave = partial_last = 0
    for which, splits in (("default", [0]), ("tuning", [1, 3, 64])):
        _ffi.select(which)
        for split in splits:
            os.environ["PVW_SUM_SPLIT"] = str(split)
            calls = 0
            for geom, (n, k, l, moduli) in enumerate(GEOMETRIES):
                p = _params(n, k, l, moduli)
                o = DeviceOut(p)
                items_a = k * p.L * l // 2
                for D in (1, 2, 7, 130, 8, 9, 63, 64, 65):
                    rng = np.random.default_rng(1000 * geom + D)
                    masks = [None, np.arange(D) % 2 == 0, np.arange(D) == D // 2, np.zeros(D, bool)]
                    ranges = [(0, n), (1, n), (n - 1, n), (0, 1)]
                    sets = _weight_sets(rng, moduli, D) + [("none", np.zeros(D, np.int64))]
                    step = 0
                    for i, kind in enumerate(["reduced", "any", "extreme"] if D in (1, 2, 7, 130) else ["any"]):
                        c1s, c2s = _words(rng, p, D, k, kind), _words(rng, p, D, n, kind)
                        d1, d2 = dev(c1s), dev(c2s)
                        for j, valid in enumerate(masks):
                            for name, w in sets:
                                if name.startswith("extreme") and name != "extreme0" and (which, kind, j) != ("default", "any", 0):
                                    continue                        # the rotations once: shipped library, any words, every dealer
                                step += 1
                                calls += 1
                                lo, hi = ranges[step % len(ranges)]
                                inside_a_wave += items_a % 64 != 0
                                partial_last += (items_a + (hi - lo) * p.L * l // 2) % 256 != 0
                                g1, g2, cnt = device_lincomb(p, o, d1, d2, D, w, valid, lo, hi, s)
                                what = (which, split, geom, D, kind, j, name, lo, hi)
                                on = int(np.count_nonzero((w != 0) & (True if valid is None else valid)))
                                assert cnt == on, what
                                if on == 0:                         # the device form combines nothing: zeros, count 0
                                    assert not g1.any() and not g2.any(), what
                                    continue
                                w1, w2 = host_lincomb(p, c1s, c2s, w, valid, lo, hi)
                                assert np.array_equal(g1, w1) and np.array_equal(g2, w2), what
                                if name == "ones":                  # every weight 1: bit-equal to the sum call, on the device too
                                    s1, s2, sc = device_sum(p, o, d1, d2, D, valid, lo, hi, s)
                                    assert np.array_equal(s1, w1) and np.array_equal(s2, w2) and sc == cnt, what
                                if which == "default" and kind != "reduced" and name in ("ones", "uniform", "extreme0", "zeros"):
                                    h1, h2, hc = hostbuf_lincomb(p, c1s, c2s, w, valid, lo, hi)
                                    assert np.array_equal(h1, w1) and np.array_equal(h2, w2) and hc == cnt, what
            print(f"combos {which} split={split} ok ({calls} device calls)", flush=True)
    os.environ.pop("PVW_SUM_SPLIT")
    _ffi.select("default")
    # the region boundary falls inside a wave and the last workgroup is partial in cases of the matrix
    assert inside_a_wave > 0 and partial_last > 0, (inside_a_wave, partial_last)
    # 130 dealers of 2^64 - 1 times INT64_MIN: every partial sum of the accumulator wraps
    p = _params(3, 2, 8, M.bench_moduli(2))
    c1s = np.full((130, p.k, p.L, p.l), (1 << 64) - 1, np.uint64)
    c2s = np.full((130, p.n, p.L, p.l), (1 << 64) - 1, np.uint64)
    w = np.full(130, I64_MIN, np.int64)
    g1, g2, cnt = device_lincomb(p, DeviceOut(p), dev(c1s), dev(c2s), 130, w, None, 0, p.n, s)
    w1, w2 = host_lincomb(p, c1s, c2s, w, None, 0, p.n)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and cnt == 130
    print("wraps ok", flush=True)


# ---- systems and the handover recipe -----------------------------------------------------------------------------------------
def system(moduli, n, k, l):
    p = _params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


class Handover:
    """The recipe of DESIGN 8.12 / INTEGRATION: the old shares sigma_d = F(d + 1) of a polynomial F of degree t are dealt
    again (pvw_deal_shares, new degree `degree`); the validity mask leaves `masked` old holders out; the weights are
    pvw_shamir_lagrange_weights over the valid old indices, 0 elsewhere.  want[j] = sum_d lambda_d f_d(j + 1) mod p from
    pvw_shamir_shares_host; exact[j] the same sum as an integer (what the plaintext of the combination is)."""

    def __init__(self, n, D, masked, k=16, l=8, t=3, degree=2, tag=0):
        self.p, self.gpk, self.parties = system(M.bench_moduli(17), n, k, l)
        rnd = random.Random(100 * n + D + tag)
        self.F = [rnd.randrange(PLAIN) for _ in range(t + 1)]
        sigma = [sum(c * pow(d + 1, e, PLAIN) for e, c in enumerate(self.F)) % PLAIN for d in range(D)]
        seeds = [api._dealer_seed(SEED, 40 + tag + d) for d in range(D)]
        self.cts = P.deal_party_shares(sigma, degree, PLAIN, self.gpk, seeds)
        self.shares = P.shamir_shares(self.p, sigma, degree, PLAIN, seeds, host=True)          # [D][n]
        self.D, self.n, self.degree = D, n, degree
        self.c1s, self.c2s = np.stack([c.c1 for c in self.cts]), np.stack([c.c2 for c in self.cts])
        self.use(masked)

    def use(self, masked):
        D = self.D
        self.valid = np.array([d not in masked for d in range(D)], np.uint8)
        on = [d for d in range(D) if self.valid[d]]
        lam = P.shamir_lagrange_weights(on, PLAIN)
        self.weights = np.zeros(D, np.int64)
        self.weights[on] = lam
        assert self.p.lincomb_fits(self.weights, self.valid)
        self.exact = [sum(int(self.weights[d]) * int(self.shares[d][j]) for d in on) for j in range(self.n)]
        self.want = [x % PLAIN for x in self.exact]
        return self


def triple(r, i=0):
    return int(r.residues[i]), int(r.noise[i]), int(r.status[i])


def decrypt():
    """the handover with t = 3, new degree 2, D = 9 old holders of which three are masked out, on both sides of the 22-party
    dispatch: the new shares are sum lambda_d pvw_shamir_shares_host[d][j] mod p bit for bit and any three reconstruct F(0);
    the one-party forms (key pointer, resident key; host buffers, device pointers) agree with the all-party form; wide
    returns |sum w_d m_d| with the sign; both options 0 give the checked word; no key material is left behind"""
    for n in (24, 6):
        h = Handover(n, 9, (1, 4, 8))
        p, parties = h.p, h.parties
        r = P.decrypt_all_party_combinations(h.cts, h.weights, parties, h.valid, plain_modulus=PLAIN)
        assert [int(x) for x in r.values] == h.want, n
        assert r.valid.all() and r.bound >= 1 << 64, n                 # by lincomb_fits: the noise word is saturated or close to it
        assert api._secret_residue(p)[0] == 0
        rnd = random.Random(n)
        for _ in range(8):
            who = rnd.sample(range(n), h.degree + 1)
            assert P.shamir_reconstruct(who, [h.want[j] for j in who], PLAIN) == h.F[0], (n, who)
        # a sub-range of parties, POWER-basis input, wide words
        lo, cnt = 1, 4
        pw = [P.PvwCiphertext(p.ntt_inverse(c.c1), p.ntt_inverse(c.c2), p, P.REPR_POWER) for c in h.cts]
        rw = P.decrypt_all_party_combinations(pw, h.weights, parties[lo:lo + cnt], h.valid, plain_modulus=PLAIN, wide=True)
        assert [int(x) for x in rw.values] == h.exact[lo:lo + cnt] and [int(x) for x in rw.residues] == h.want[lo:lo + cnt], n
        assert [bool(x) for x in rw.negative] == [x < 0 for x in h.exact[lo:lo + cnt]] and not rw.truncated.any(), n
        assert api._secret_residue(p)[0] == 0
        # one party: host buffers; device pointers with the key's coefficients and with the resident key
        W = (p.q_total().bit_length() + 63) // 64
        c1, dv, dw = dev(h.c1s), dev(h.valid), dev(h.weights)
        for i in (0, 3, n - 1):
            one = P.decrypt_party_combination(h.cts, h.weights, parties[i].secret_key, i, h.valid, plain_modulus=PLAIN, wide=True)
            assert int(one.residues[0]) == h.want[i] and int(one.values[0]) == h.exact[i], (n, i)
            assert (int(one.noise[0]), int(one.status[0])) == (int(r.noise[i]), int(r.status[i])), (n, i)
            assert api._secret_residue(p)[0] == 0
            col = dev(np.ascontiguousarray(h.c2s[:, i]))
            for resident in (False, True):
                out, nz = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
                st, dc = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
                wide = torch.zeros(W, dtype=torch.int64, device=DEV)
                noisy = torch.zeros((p.L, p.l), dtype=torch.int64, device=DEV)
                torch.cuda.synchronize()
                if resident:
                    with P.DeviceSecretKey(parties[i].secret_key) as key:
                        key.decrypt_lincomb_device_plain(c1, col, h.D, dw, out, d_valid=dv, d_noisy=noisy, d_noise=nz, d_status=st,
                                                         d_count=dc, stream=torch.cuda.current_stream(), plain_modulus=PLAIN, wide=wide,
                                                         wide_words=W)
                        torch.cuda.synchronize()
                else:
                    sk = dev(parties[i].secret_key.secret_coeffs.astype(np.int64))
                    p._call("pvw_decrypt_lincomb_plain_device", ptr(sk), ptr(c1), ptr(col), h.D, ptr(dv), ptr(dw), P.REPR_NTT, ptr(noisy),
                            ptr(out), ptr(nz), ptr(st), ptr(dc), PLAIN, W, ptr(wide), cur())
                    torch.cuda.synchronize()
                assert (int(u64(out)[0]), int(u64(nz)[0]), int(st.item())) == triple(one), (n, i, resident)
                assert int(dc.item()) == 6, (n, i, resident)
                mag = sum(int(x) << (64 * j) for j, x in enumerate(u64(wide)))
                assert (-mag if int(st.item()) & api.DEC_NEGATIVE else mag) == h.exact[i], (n, i, resident)
                # the noisy polynomial handed out decodes on the host to the same report, plain and checked
                ref = P.decode_scalar_pvw_plain_host(p, u64(noisy)[None], plain_modulus=PLAIN)
                assert triple(ref) == triple(one), (n, i, resident)
                assert api._secret_residue(p)[0] == 0
            # both options 0: the checked word of the same noisy polynomial
            chk = P.decrypt_party_combination(h.cts, h.weights, parties[i].secret_key, i, h.valid)
            ref = P.decode_scalar_pvw_checked_host(p, u64(noisy)[None])
            assert triple(chk) == triple(ref), (n, i)
        # a masked-out dealer is not read even where its weight is not 0; a valid dealer of weight 0 does not count
        w2 = h.weights.copy()
        w2[1] = 12345
        r2 = P.decrypt_all_party_combinations(h.cts, w2, parties, h.valid, plain_modulus=PLAIN)
        assert [int(x) for x in r2.values] == h.want, n
        # small weights: the noise word is meaningful and inside count * sum |w| bounds
        small = np.array([2, -1, 0, 3, 1, -2, 0, 1, -1], np.int64)
        rs = P.decrypt_all_party_combinations(h.cts, small, parties, None, plain_modulus=PLAIN)
        assert [int(x) for x in rs.values] == [sum(int(small[d]) * int(h.shares[d][j]) for d in range(h.D)) % PLAIN for j in range(n)], n
        assert rs.valid.all() and rs.bound == 11 * p.noise_bound() and int(rs.noise.max()) <= rs.bound, n
        assert api._secret_residue(p)[0] == 0
        print(f"decrypt n={n} ok", flush=True)


# ---- pieces ------------------------------------------------------------------------------------------------------------------
class budget:
    """PVW_STAGE_BYTES around one call (None: unset, the default of 1 GiB)"""

    def __init__(self, b):
        self.b = b

    def __enter__(self):
        os.environ.pop("PVW_STAGE_BYTES", None)
        if self.b is not None:
            os.environ["PVW_STAGE_BYTES"] = str(self.b)

    def __exit__(self, *exc):
        os.environ.pop("PVW_STAGE_BYTES", None)


def fills(part, per):
    """ct_sum_staged: the dealers combined by each launch (part[d]: dealer d takes part)"""
    out, fill, d, D = [], 0, 0, len(part)
    while d < D:
        if not part[d]:
            d += 1
            continue
        run = 1
        while d + run < D and fill + run < per and part[d + run]:
            run += 1
        fill, d = fill + run, d + run
        if fill == per:
            out.append(fill)
            fill = 0
    return out + ([fill] if fill else [])


def pieces():
    """the tuning build with PVW_STAGE_BYTES so small that pvw_ct_lincomb, pvw_decrypt_lincomb_plain and
    pvw_decrypt_all_lincomb_plain each take three or four pieces (the accumulate path, every piece with its own weights) at
    n = 8, D = 13: bit-equal to one piece and to the references"""
    _ffi.select("tuning")
    n, D = 8, 13
    h = Handover(n, D, (2, 5, 6, 11), tag=7)
    p, parties = h.p, h.parties
    Pw = p.L * p.l
    part = (h.valid != 0) & (h.weights != 0)
    nv = int(part.sum())
    assert nv == 9

    def budget_for(item, per):
        b = per * item + item // 2
        f = fills(part, min(max(b // item, 1), nv))
        assert len(f) >= 3 and max(f) == per, f
        return b, f

    # pvw_ct_lincomb, rows [1, n): uniform int64 weights with zeros, any words
    rng = np.random.default_rng(5)
    w = rng.integers(I64_MIN, I64_MAX, D, dtype=np.int64, endpoint=True)
    w[h.weights == 0] = 0
    w[2] = 77                                                            # masked out: not read whatever its weight
    w[7] = 0                                                             # valid, weight 0: not staged either
    part = (h.valid != 0) & (w != 0)
    nv = int(part.sum())
    assert nv == 8
    c1s, c2s = _words(rng, p, D, p.k, "any"), _words(rng, p, D, n, "any")
    w1, w2 = host_lincomb(p, c1s, c2s, w, h.valid, 1, n)
    for per in (3, 2):
        b, f = budget_for((p.k + n - 1) * Pw * 8, per)
        for bb in (None, b):
            with budget(bb):
                g1, g2, cnt = hostbuf_lincomb(p, c1s, c2s, w, h.valid, 1, n)
            assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and cnt == nv, ("ct_lincomb", per, bb)
        print(f"pieces ct_lincomb: {f}", flush=True)
    # the decrypts: the handover's new shares
    part = (h.valid != 0) & (h.weights != 0)
    nv = int(part.sum())
    b, f = budget_for((p.k + 1) * Pw * 8, 3)
    for i in (0, n - 1):
        got = []
        for bb in (None, b):
            with budget(bb):
                r = P.decrypt_party_combination(h.cts, h.weights, parties[i].secret_key, i, h.valid, plain_modulus=PLAIN, wide=True)
            got.append((triple(r), int(r.values[0])))
            assert api._secret_residue(p)[0] == 0
        assert got[0] == got[1] and got[0][0][0] == h.want[i] and got[0][1] == h.exact[i], ("one party", i, got)
    print(f"pieces decrypt_lincomb_plain: {f}", flush=True)
    for lo, cnt in ((0, n), (2, 3)):
        b, f = budget_for((p.k + cnt) * Pw * 8, 3)
        got = []
        for bb in (None, b):
            with budget(bb):
                r = P.decrypt_all_party_combinations(h.cts, h.weights, parties[lo:lo + cnt], h.valid, plain_modulus=PLAIN)
            got.append([triple(r, j) for j in range(cnt)])
            assert api._secret_residue(p)[0] == 0
        assert got[0] == got[1] and [x[0] for x in got[0]] == h.want[lo:lo + cnt], ("all parties", lo, cnt)
        print(f"pieces decrypt_all_lincomb_plain [{lo}, {lo + cnt}): {f}", flush=True)
    _ffi.select("default")


def big():
    """one production shape: config-3 geometry (k = 256, l = 8, 17 moduli), 256 parties' rows, D = 128, any 64-bit words,
    uniform int64 weights with a quarter of the dealers masked out, against pvw_ct_lincomb_host"""
    n, k, l, D = 256, 256, 8, 128
    p = _params(n, k, l, M.bench_moduli(17))
    s = torch.cuda.Stream(device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(D + n)
    d1 = torch.empty((D, k, p.L, l), dtype=torch.int64, device=DEV).random_(generator=g)
    d2 = torch.empty((D, n, p.L, l), dtype=torch.int64, device=DEV).random_(generator=g)
    for t in (d1, d2):                                           # random_ leaves bit 63 clear
        t.bitwise_xor_(t.bitwise_left_shift(13))
    valid = np.arange(D) % 4 != 1
    w = np.random.default_rng(9).integers(I64_MIN, I64_MAX, D, dtype=np.int64, endpoint=True)
    w1, w2 = host_lincomb(p, u64(d1), u64(d2), w, valid, 0, n)
    g1, g2, cnt = device_lincomb(p, DeviceOut(p), d1, d2, D, w, valid, 0, n, s)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and cnt == 96
    print("big ok", flush=True)


def capture():
    """after pvw_prepare(PVW_PREPARE_SUM) a captured pvw_decrypt_all_lincomb_plain_device replays with changed weights and a
    changed mask, and every replay equals the eager call; without pvw_prepare the call is refused by name and the capture
    survives"""
    lib = _ffi.lib()
    n, D = 24, 9
    h = Handover(n, D, (1, 4, 8), tag=3)
    p, parties = h.p, h.parties
    W = (p.q_total().bit_length() + 63) // 64
    c1, c2 = dev(h.c1s), dev(h.c2s)
    sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
    mask, weights = dev(h.valid), dev(h.weights)

    class Out:
        def __init__(self):
            self.out, self.noise = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
            self.status, self.count = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            self.wide = torch.zeros((n, W), dtype=torch.int64, device=DEV)

        def rows(self):
            return (u64(self.out).tolist(), u64(self.noise).tolist(), self.status.cpu().tolist(), int(self.count.item()), u64(self.wide).tolist())

    def enqueue(o, cs):
        rc = lib.pvw_decrypt_all_lincomb_plain_device(p._h, 0, n, ptr(sk), ptr(c1), ptr(c2), D, ptr(mask), ptr(weights), P.REPR_NTT,
                                                      ptr(o.out), ptr(o.noise), ptr(o.status), ptr(o.count), PLAIN, W, ptr(o.wide), cs)
        return rc, _ffi.last_error(lib)

    captured, eager = Out(), Out()
    s0 = torch.cuda.Stream(device=DEV)                                    # not prepared: a stream the context has never seen
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s0):
        rc, msg = enqueue(captured, cur())
    torch.cuda.synchronize()
    assert rc == 1 and "pvw_prepare" in msg, (rc, msg)
    del g0
    s = torch.cuda.Stream(device=DEV)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, msg = enqueue(captured, cur())
    assert rc == 0, msg
    for rep, masked in enumerate(((1, 4, 8), (0, 2, 3, 7), ())):
        h.use(masked)
        if rep == 2:                                                       # small weights, one of them 0: no Lagrange set
            h.weights = np.array([3, -2, 0, 1, 1, -5, 2, 0, 4], np.int64)
            h.want = [sum(int(h.weights[d]) * int(h.shares[d][j]) for d in range(D)) % PLAIN for j in range(n)]
        mask.copy_(torch.from_numpy(h.valid))
        weights.copy_(torch.from_numpy(h.weights))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rc, msg = enqueue(eager, cur())
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert captured.rows() == eager.rows(), rep
        assert captured.rows()[0] == h.want and captured.rows()[3] == int(np.count_nonzero((h.valid != 0) & (h.weights != 0))), rep
    del g
    assert api._secret_residue(p)[0] == 0
    print("capture ok", flush=True)


def threads():
    """two threads on one context call pvw_ct_lincomb / pvw_decrypt_lincomb_plain / pvw_decrypt_all_lincomb_plain at the same
    time, round after round: every result is the serial one"""
    n, D = 6, 9
    h = Handover(n, D, (1, 4, 8), tag=5)
    p, parties = h.p, h.parties
    rng = np.random.default_rng(8)
    w = rng.integers(I64_MIN, I64_MAX, D, dtype=np.int64, endpoint=True)
    w[3] = 0
    c1s, c2s = _words(rng, p, D, p.k, "any"), _words(rng, p, D, n, "any")

    def job_comb():
        return tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in hostbuf_lincomb(p, c1s, c2s, w, h.valid, 1, n))

    def job_one(i):
        return triple(P.decrypt_party_combination(h.cts, h.weights, parties[i].secret_key, i, h.valid, plain_modulus=PLAIN))

    def job_all():
        r = P.decrypt_all_party_combinations(h.cts, h.weights, parties, h.valid, plain_modulus=PLAIN)
        return [triple(r, j) for j in range(n)]

    plans = [[job_comb, lambda: job_one(2), job_all, job_comb, lambda: job_one(5)],
             [lambda: job_one(4), job_comb, job_comb, job_all, job_all]]
    serial = [[job() for job in plan] for plan in plans]
    assert serial[0][1][0] == h.want[2] and [x[0] for x in serial[0][2]] == h.want
    rounds = 6
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


CASES = {f.__name__: f for f in (combos, pieces, big, decrypt, capture, threads)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("CT_LINCOMB_OK")

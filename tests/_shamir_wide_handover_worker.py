"""The wide handover on the device: the signed-digit, weights and fold kernels bit for bit against their _host
forms, and pvw_decrypt_all_handover_wide* against the Python truth from host shares and against the composition
pvw_shamir_wide_handover_weights_host -> pvw_decrypt_all_lincomb_many_plain -> pvw_shamir_wide_from_digits_host; hygiene, staging
in pieces, stream capture, two threads.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_shamir_wide_handover.py; prints SHAMIR_WIDE_HANDOVER_OK."""
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
from test_shamir_wide_host import SECP_N, ints  # noqa: E402
from test_shamir_wide_handover_host import edge_set, lagrange_at  # noqa: E402
from _ct_lincomb_worker import budget, cur, dev, ptr, system, u64  # noqa: E402
from _shamir_wide_worker import _params  # noqa: E402

DEV = torch.device("cuda", 0)
P17, P65, P255 = 65537, 2**64 + 13, 2**255 - 19
PRIMES4 = (P17, P65, P255, SECP_N)
MARK = -0x5A5A5A5A5A5A5A5B


def clean(st):
    """no status bit but DEC_LOSSY, which only says that a digit plaintext is no uint64 (informational with wide words)"""
    return not (np.asarray(st) & ~np.uint32(P.DEC_LOSSY)).any()


def digits():
    """pvw_shamir_wide_signed_digits_device == the host rule on the edge set, N on either side of a wave and of a workgroup"""
    p = _params(3)
    rng = random.Random(1)
    for pm in PRIMES4:
        for b in (8, 33, 60, 64):
            for N in (1, 63, 64, 65, 257):
                vals = (edge_set(pm, b) + [rng.getrandbits(256) for _ in range(N)])[:N] if N > 1 else [pm // 2 + 1]
                got = P.shamir_wide_signed_digits(p, vals, pm, b)
                assert np.array_equal(got, P.shamir_wide_signed_digits(None, vals, pm, b, host=True)), (pm, b, N)
    print("digits ok", flush=True)


def device_weights(p, idx, pm, valid, points, lb, b, stream=None):
    """pvw_shamir_wide_handover_weights_device into the middle of a marked buffer: (rows, the guard words are intact)"""
    D = len(idx)
    NL, V = P.shamir_wide_handover_shape(pm, lb, b)
    T = 1 if points is None else len(points)
    words, pad = T * V * D * NL, 1024
    buf = torch.full((words + 2 * pad,), MARK, dtype=torch.int64, device=DEV)
    ix = np.array(idx, dtype=np.uint64)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    pts = None if points is None else api._wide(points)
    s = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    p._call("pvw_shamir_wide_handover_weights_device", api._ptr(api._wide_modulus(pm)), api._ptr(ix), api._ptr(v), D, api._ptr(pts), T, lb, b,
            C.c_void_p(buf.data_ptr() + pad * 8), C.c_void_p(s.cuda_stream))
    s.synchronize()
    a = buf.cpu().numpy()
    return a[pad:pad + words].reshape(T * V, D * NL), bool((a[:pad] == MARK).all() and (a[pad + words:] == MARK).all())


def weights():
    """the weight rows == the host rows, written into a marked buffer: D across the 32-column batch and the 64-lane wave, masks
    (first, last, alternating, one valid), T on either side of a wave, targets on valid and on masked holders, four primes, both
    limb widths, four digit widths; the masked columns are 0 and nothing outside the matrix is written"""
    p = _params(3)
    rng = random.Random(2)
    s = torch.cuda.Stream(device=DEV)
    shapes = [(52, 64), (62, 33), (52, 8), (62, 60), (52, 60), (62, 64), (52, 33), (62, 8)]
    case = 0
    for D in (1, 2, 5, 33, 65, 130):
        masks = [None, [d != 0 for d in range(D)], [d != D - 1 for d in range(D)], [d % 2 == 0 for d in range(D)], [d == D // 2 for d in range(D)]]
        for mi, valid in enumerate(masks):
            if valid is not None and not any(valid):
                continue
            for T in (1, 2, 63, 64, 65):
                if D >= 65 and T >= 63 and mi not in (0, 3):
                    continue
                pm = PRIMES4[case % 4]
                lb, b = shapes[(case // 4 + case) % 8]
                case += 1
                if D >= 33 and T >= 63 and b == 8:
                    b = 60
                idx = rng.sample(range(min(pm - 2, 4000)), D)
                on = [d for d in range(D) if valid is None or valid[d]]
                off = [d for d in range(D) if d not in on]
                points = None
                if T > 1 or case % 2:
                    points = [rng.randrange(pm) for _ in range(T)]
                    points[0] = idx[on[-1]] + 1                           # on a valid holder
                    if T > 1:
                        points[1] = idx[off[0]] + 1 if off else 0         # on a masked holder: an ordinary point
                    if T > 2:
                        points[2], points[-1] = 0, pm - 1
                got, intact = device_weights(p, idx, pm, valid, points, lb, b, s)
                want = P.shamir_wide_handover_weights(None, idx, pm, valid, points, lb, b, host=True)
                assert intact and np.array_equal(got, want), (D, mi, T, pm, lb, b)
                NL = P.shamir_wide_handover_shape(pm, lb, b)[0]
                for d in off:
                    assert not got[:, d * NL:(d + 1) * NL].any(), (D, mi, T, d)
        print(f"weights D={D} ok", flush=True)
    # the api's device form
    idx = [3, 0, 9, 4]
    assert np.array_equal(P.shamir_wide_handover_weights(p, idx, SECP_N, [1, 1, 0, 1], [0, SECP_N - 1]),
                          P.shamir_wide_handover_weights(None, idx, SECP_N, [1, 1, 0, 1], [0, SECP_N - 1], host=True))
    print("weights ok", flush=True)


def fold():
    """pvw_shamir_wide_from_digits_device == the host fold over a [P][T V] report read in place, count = P T on either side of a
    workgroup; every ww and the digit widths on both sides of the 31-bit multiplier steps"""
    p = _params(3)
    rng = np.random.default_rng(3)
    case = 0
    for count in (1, 255, 256, 257):
        for pm in PRIMES4:
            for ww in (1, 2, 3, 4):
                b = (8, 31, 32, 33, 60, 62, 63, 64)[case % 8]
                case += 1
                V = P.shamir_wide_handover_shape(pm, 62, b)[1]
                wide = rng.integers(0, 1 << 63, (count, V, ww), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (count, V, ww), dtype=np.uint64)
                status = rng.integers(0, 8, (count, V), dtype=np.uint32)
                wide[0] = 0
                got = P.shamir_wide_from_digits(p, wide, status, pm, b)
                want = P.shamir_wide_from_digits(None, wide, status, pm, b, host=True)
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (count, pm, ww, b)
    print("fold ok", flush=True)


class WideHandover:
    """An old sharing over the secp256k1 order whose D = 6 holders re-deal their shares limb by limb (deal_party_shares_wide, new
    degree 2, 52-bit limbs) to n new parties; holder 1 is masked out.  pack = 1: a degree-2 sharing of one secret at the point 0;
    pack = 3: a packed sharing (degree 4) of three secrets at the points 0, -1, -2.  truth[j][m] = sum_d lambda_{d,m} f_d(j + 1)
    mod p from pvw_shamir_shares_wide_host."""
    IDX, VALID, DEGREE, LB = [0, 5, 2, 7, 3, 9], [1, 0, 1, 1, 1, 1], 2, 52

    def __init__(self, n, pack=1, tag=0, system_=None):
        self.p, self.gpk, self.parties = system_ or system(M.bench_moduli(17), n, 16, 8)
        self.n, self.pm, self.pack = n, SECP_N, pack
        pm, D = self.pm, len(self.IDX)
        rnd = random.Random(1000 * n + 10 * pack + tag)
        self.secrets = [rnd.randrange(pm) for _ in range(pack)]
        old = _params(10)
        if pack == 1:
            y = ints(P.shamir_shares_wide(old, self.secrets, 2, pm, seeds=[bytes([tag + 1]) * 32], host=True))[0]
            self.points = None
        else:
            y = ints(P.shamir_shares_packed_wide(old, [self.secrets], pack, 2, pm, seeds=[bytes([tag + 1]) * 32], host=True))[0]
            self.points = P.shamir_packed_wide_handover_points(pm, pack)
        mine = [y[i] for i in self.IDX]
        self.NL = P.shamir_wide_limbs(pm, self.LB)
        seeds = [api._dealer_seed(bytes([0x2C]) * 32, 100 * tag + v) for v in range(D * self.NL)]
        self.cts = P.deal_party_shares_wide(mine, self.DEGREE, pm, self.gpk, seeds=seeds, limb_bits=self.LB)
        self.shares = ints(P.shamir_shares_wide(self.p, mine, self.DEGREE, pm, seeds=seeds[::self.NL], host=True))      # [D][n]
        flat = [ct for row in self.cts for ct in row]
        self.c1s, self.c2s = np.stack([c.c1 for c in flat]), np.stack([c.c2 for c in flat])
        on = [d for d in range(D) if self.VALID[d]]
        self.truth = []
        for j in range(n):
            row = []
            for pt in (self.points or [0]):
                lam = lagrange_at(pm, [self.IDX[d] + 1 for d in on], pt)
                row.append(sum(a * self.shares[d][j] for a, d in zip(lam, on)) % pm)
            self.truth.append(row)

    def composition(self, b, lo, hi, repr_=P.REPR_NTT, c1s=None, c2s=None):
        """weights_host -> pvw_decrypt_all_lincomb_many_plain -> from_digits_host: (values [P][T], status [P][T])"""
        p, D, NP = self.p, len(self.IDX), hi - lo
        rows = P.shamir_wide_handover_weights(None, self.IDX, self.pm, self.VALID, self.points, self.LB, b, host=True)
        R = len(rows)
        V = P.shamir_wide_handover_shape(self.pm, self.LB, b)[1]
        ww = -(-(self.LB + b + (sum(self.VALID) * self.NL - 1).bit_length() + 1) // 64)
        out, st, wide = np.zeros((NP, R), np.uint64), np.zeros((NP, R), np.uint32), np.zeros((NP, R, ww), np.uint64)
        sk = np.ascontiguousarray(np.stack([pt.secret_key.secret_coeffs for pt in self.parties[lo:hi]]).astype(np.int64))
        c1s, c2s = (self.c1s if c1s is None else c1s), (self.c2s if c2s is None else c2s)
        p._call("pvw_decrypt_all_lincomb_many_plain", lo, hi, api._ptr(sk), api._ptr(c1s), api._ptr(c2s), D * self.NL, None, api._ptr(rows), R,
                repr_, api._ptr(out), None, api._ptr(st), None, 0, ww, api._ptr(wide))
        vals, so = P.shamir_wide_from_digits(None, wide.reshape(NP, R // V, V, ww), st.reshape(NP, R // V, V), self.pm, b, host=True)
        T = R // V
        return [vals[j * T:(j + 1) * T] for j in range(NP)], so

    def device(self, b, lo, hi, bufs, repr_=P.REPR_NTT, stream=None, digit_bits=None):
        """pvw_decrypt_all_handover_wide_device on buffers made by device_buffers: rc and the message"""
        lib = _ffi.lib()
        ix = np.array(self.IDX, dtype=np.uint64)
        v = np.array(self.VALID, dtype=np.uint8)
        pts = None if self.points is None else api._wide(self.points)
        T = 1 if pts is None else len(pts)
        rc = lib.pvw_decrypt_all_handover_wide_device(self.p._h, lo, hi, ptr(bufs["sk"]), ptr(bufs["c1"]), ptr(bufs["c2"]), len(self.IDX),
                                                      api._ptr(api._wide_modulus(self.pm)), self.LB, b if digit_bits is None else digit_bits,
                                                      api._ptr(ix), api._ptr(v), api._ptr(pts), T, repr_, ptr(bufs["out"]), ptr(bufs["st"]),
                                                      ptr(bufs["cnt"]), stream or cur())
        return rc, _ffi.last_error(lib)

    def device_buffers(self, lo, hi, c1s=None, c2s=None):
        T = 1 if self.points is None else len(self.points)
        sk = np.stack([pt.secret_key.secret_coeffs for pt in self.parties[lo:hi]]).astype(np.int64)
        return {"sk": dev(sk), "c1": dev(self.c1s if c1s is None else c1s), "c2": dev(self.c2s if c2s is None else c2s),
                "out": torch.full((hi - lo, T, 4), -1, dtype=torch.int64, device=DEV), "st": torch.full((hi - lo, T), -1, dtype=torch.int32, device=DEV),
                "cnt": torch.full((1,), -1, dtype=torch.int32, device=DEV)}


def values_of(bufs):
    out = u64(bufs["out"])
    return [ints(out[j]) for j in range(out.shape[0])]


def handover():
    """n = 12 (per-party path) and n = 24 (GEMM path), b = 60 and 64: wide_handover_fits holds; the one call gives the Python truth,
    equals the composition of the three pieces bit for bit, t + 1 new shares reconstruct the old secret; both representations, a
    sub-range of parties, the device form; a packed old sharing at the points 0, -1, -2"""
    for n in (12, 24):
        for pack in (1, 3):
            h = WideHandover(n, pack)
            p, pm = h.p, h.pm
            rnd = random.Random(n + pack)
            pw = [[P.PvwCiphertext(p.ntt_inverse(c.c1), p.ntt_inverse(c.c2), p, P.REPR_POWER) for c in row] for row in h.cts]
            for b in (60, 64):
                assert p.wide_handover_fits(pm, sum(h.VALID), h.LB, b), (n, b)
                vals, st = P.decrypt_all_party_handover_wide(h.cts, h.parties, h.IDX, pm, h.VALID, h.points, h.LB, b)
                assert vals == h.truth and clean(st), (n, pack, b)
                cv, cs = h.composition(b, 0, n)
                assert vals == cv and np.array_equal(st, cs), (n, pack, b)
                assert api._secret_residue(p)[0] == 0
                for m in range(pack):
                    for _ in range(3):
                        who = rnd.sample(range(n), h.DEGREE + 1)
                        assert P.shamir_reconstruct_wide(who, [vals[j][m] for j in who], pm) == h.secrets[m], (n, pack, b, m)
                # POWER-basis input and a sub-range of parties
                lo, cnt = 1, 4
                vals2, st2 = P.decrypt_all_party_handover_wide(pw, h.parties[lo:lo + cnt], h.IDX, pm, h.VALID, h.points, h.LB, b)
                assert vals2 == h.truth[lo:lo + cnt] and clean(st2), (n, pack, b)
                # device pointers, both representations
                for repr_, c1s, c2s in ((P.REPR_NTT, None, None),
                                        (P.REPR_POWER, np.stack([c.c1 for r in pw for c in r]), np.stack([c.c2 for r in pw for c in r]))):
                    for lo, hi in ((0, n), (2, 7)):
                        bufs = h.device_buffers(lo, hi, c1s, c2s)
                        torch.cuda.synchronize()
                        rc, msg = h.device(b, lo, hi, bufs, repr_)
                        assert rc == 0, msg
                        torch.cuda.synchronize()
                        assert values_of(bufs) == h.truth[lo:hi] and clean(bufs["st"].cpu().numpy().view(np.uint32)), (n, pack, b, repr_, lo)
                        assert bufs["cnt"].cpu().tolist() == [sum(h.VALID)]
                        assert api._secret_residue(p)[0] == 0
            print(f"handover n={n} pack={pack} ok", flush=True)


def hygiene():
    """pvw_selftest_secret_residue is 0 after a successful call of either form and after a refusal"""
    for n in (12, 24):
        h = WideHandover(n, tag=2)
        p = h.p
        vals, _ = P.decrypt_all_party_handover_wide(h.cts, h.parties, h.IDX, h.pm, h.VALID, None, h.LB, 64)
        assert vals == h.truth and api._secret_residue(p)[0] == 0
        try:
            P.decrypt_all_party_handover_wide(h.cts, h.parties, [0, 5, 2, 7, 3, 3], h.pm, None, None, h.LB, 64)     # a duplicate holder
            raise AssertionError("not refused")
        except P.PvwError as e:
            assert e.code == 1
        assert api._secret_residue(p)[0] == 0
        bufs = h.device_buffers(0, n)
        torch.cuda.synchronize()
        rc, msg = h.device(60, 0, n, bufs)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert values_of(bufs) == h.truth and api._secret_residue(p)[0] == 0
        marked = {k_: v.clone() for k_, v in bufs.items()}
        rc, msg = h.device(60, 0, n, bufs, digit_bits=7)
        torch.cuda.synchronize()
        assert rc == 1 and all(torch.equal(bufs[k_], marked[k_]) for k_ in bufs) and api._secret_residue(p)[0] == 0
    print("hygiene ok", flush=True)


def pieces():
    """the tuning build with PVW_STAGE_BYTES so small that the many-combinations pass inside the host-buffer call stages its 25
    participating vectors in several pieces: the same values as in one piece"""
    _ffi.select("tuning")
    n = 12
    h = WideHandover(n, tag=3)
    p = h.p
    item = (p.k + n) * p.L * p.l * 8
    got = []
    for bb in (None, 7 * item + item // 2, 2 * item + item // 2):
        with budget(bb):
            got.append(P.decrypt_all_party_handover_wide(h.cts, h.parties, h.IDX, h.pm, h.VALID, None, h.LB, 64))
        assert api._secret_residue(p)[0] == 0
    for vals, st in got:
        assert vals == h.truth and clean(st)
    _ffi.select("default")
    print("pieces ok", flush=True)


def capture():
    """the device form is refused under capture on a stream nothing has sized, with nothing enqueued; after a call outside capture
    it is captured and replayed twice with other ciphertexts"""
    n = 12
    sysm = system(M.bench_moduli(17), n, 16, 8)
    hs = [WideHandover(n, tag=4 + i, system_=sysm) for i in range(3)]
    h = hs[0]
    p = h.p
    bufs = h.device_buffers(0, n)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s):
        rc, msg = h.device(64, 0, n, bufs)
    torch.cuda.synchronize()
    assert rc == 1 and "outside capture first" in msg, (rc, msg)
    g0.replay()
    torch.cuda.synchronize()
    assert (bufs["out"] == -1).all() and (bufs["st"] == -1).all() and (bufs["cnt"] == -1).all()
    del g0
    with torch.cuda.stream(s):
        rc, msg = h.device(64, 0, n, bufs)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert values_of(bufs) == h.truth
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, msg = h.device(64, 0, n, bufs)
    assert rc == 0, msg
    for other in hs[1:]:
        bufs["c1"].copy_(dev(other.c1s))
        bufs["c2"].copy_(dev(other.c2s))
        bufs["out"].fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert values_of(bufs) == other.truth and clean(bufs["st"].cpu().numpy().view(np.uint32)) and bufs["cnt"].cpu().tolist() == [5]
    del g
    assert api._secret_residue(p)[0] == 0
    print("capture ok", flush=True)


def threads():
    """two threads on one context call the host-buffer form next to each other (b = 64 and b = 60, all parties and a sub-range):
    every result is the serial twin's"""
    n = 12
    h = WideHandover(n, tag=8)
    p = h.p

    def job(b, lo, hi):
        vals, st = P.decrypt_all_party_handover_wide(h.cts, h.parties[lo:hi], h.IDX, h.pm, h.VALID, None, h.LB, b)
        return vals, st.tolist()

    plans = [[(64, 0, n), (60, 2, 7), (64, 0, n)], [(60, 0, n), (64, 0, n), (60, 1, 5)]]
    serial = [[job(*a) for a in plan] for plan in plans]
    assert serial[0][0][0] == h.truth and serial[1][2][0] == h.truth[1:5]
    rounds = 3
    barrier = threading.Barrier(2)
    got, errors = [[], []], []

    def work(t):
        try:
            for _ in range(rounds):
                for a in plans[t]:
                    barrier.wait(timeout=60)
                    got[t].append(job(*a))
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


CASES = {f.__name__: f for f in (digits, weights, fold, handover, hygiene, pieces, capture, threads)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_WIDE_HANDOVER_OK")

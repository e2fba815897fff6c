"""The one-word handover with weights from a device-side mask on the device: the weights kernels and the mask kernel
bit for bit against their _host forms, and pvw_decrypt_all_handover* against the composition pvw_shamir_handover_weights_host ->
pvw_decrypt_all_lincomb_many_plain and against the Python truth from host shares; the mask changed in device memory between two
calls and between two replays of one captured call; corrected reconstruction -> mask -> handover without a host read; hygiene,
staging and target groups in pieces, two threads.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case
by case by tests/test_gpu_shamir_handover.py; prints SHAMIR_HANDOVER_OK."""
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
from test_shamir_host import P31, P62  # noqa: E402
from test_shamir_handover_host import indices_for, mask_ref, masks_for, weights_ref  # noqa: E402
from _ct_lincomb_worker import budget, cur, dev, ptr, system, u64  # noqa: E402
from _shamir_wide_worker import _params  # noqa: E402

DEV = torch.device("cuda", 0)
PLAIN = (1 << 61) - 1
MARK = -0x5A5A5A5A5A5A5A5B


def device_weights(p, idx, pm, valid, targets, stream=None):
    """pvw_shamir_handover_weights_device into the middle of a marked buffer, the mask in device memory: (rows, count, the guard
    words are intact)"""
    D, T = len(idx), 1 if targets is None else len(targets)
    words, pad = T * D, 1024
    buf = torch.full((words + 2 * pad,), MARK, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ix = np.array(idx, dtype=np.uint64)
    dv = None if valid is None else torch.tensor([0x80 if v else 0 for v in valid], dtype=torch.uint8, device=DEV)   # any byte but 0 is valid
    tg = None if targets is None else np.array(targets, dtype=np.uint64)
    s = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    p._call("pvw_shamir_handover_weights_device", pm, api._ptr(ix), ptr(dv), D, api._ptr(tg), T, C.c_void_p(buf.data_ptr() + pad * 8),
            ptr(cnt), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()                                          # the default stream's handle is NULL: the context's own stream
    a = buf.cpu().numpy()
    return a[pad:pad + words].reshape(T, D), int(cnt.item()), bool((a[:pad] == MARK).all() and (a[pad + words:] == MARK).all())


def weights():
    """the weight rows == the host rows, every word written and none outside: D on either side of the 8-column Cauchy batch, the
    64-lane wave and the 256-point upload; no mask, one holder masked, one holder valid, all masked, only holders beyond lane 63;
    T in {1 (NULL targets), 3, 65}; targets on valid and on masked holders, the points 0 and -m; three primes"""
    p = _params(3)
    rng = random.Random(2)
    s = torch.cuda.Stream(device=DEV)
    primes = (65537, P31, P62)
    case = 0
    for D in (1, 2, 7, 8, 9, 63, 64, 65, 257):
        masks = masks_for(D) + ([[int(d >= 64) for d in range(D)]] if D > 64 else [])
        for valid in masks:
            for T in (1, 3, 65):
                pm = primes[case % 3]
                case += 1
                idx = indices_for(D, pm, rng)
                on = [d for d in range(D) if valid is None or valid[d]]
                off = [d for d in range(D) if d not in on]
                targets = None
                if T > 1:
                    targets = [rng.randrange(pm) for _ in range(T)]
                    targets[0] = pm - 1 - case % 3                        # the points 0, -1, -2
                    targets[1] = idx[on[-1]] if on else pm - 2            # on a valid holder: its unit vector
                    targets[2] = idx[off[0]] if off else pm - 3           # on a masked holder: an ordinary point
                got, count, intact = device_weights(p, idx, pm, valid, targets, s)
                want, wcount = P.shamir_handover_weights(None, idx, pm, valid, targets, host=True)
                assert intact and count == wcount == len(on), (D, valid and sum(valid), T, pm)
                assert np.array_equal(got, want), (D, valid and sum(valid), T, pm)
                for d in off:
                    assert not got[:, d].any()
                if T > 1 and on:
                    assert got[1].tolist() == [int(d == on[-1]) for d in range(D)]
        print(f"weights D={D} ok", flush=True)
    # against Lagrange in Python integers once, and the api's device forms (a host mask uploaded, a device mask in place)
    idx, valid, targets = [3, 0, 9, 4], [1, 1, 0, 1], [P62 - 1, 9, 3, P62 - 2]
    got, count = P.shamir_handover_weights(p, idx, P62, valid, targets)
    assert got.tolist() == weights_ref(P62, idx, valid, targets) and count == 3
    dw, dc = P.shamir_handover_weights(p, idx, P62, torch.tensor(valid, dtype=torch.uint8, device=DEV), targets)
    torch.cuda.synchronize()
    assert np.array_equal(dw.cpu().numpy(), got) and dc.item() == 3
    print("weights ok", flush=True)


def mask():
    """pvw_shamir_valid_mask_device == the host form on both layouts, counts on either side of a wave and of a workgroup, either
    array NULL, a marked output"""
    p = _params(3)
    lib = _ffi.lib()
    rng = random.Random(5)
    for rows, count in ((1, 1), (1, 63), (1, 64), (1, 65), (3, 257), (12, 6), (24, 70)):
        status = np.array([[rng.choice([0, 0, 0, 0, 1, 2, 4, 6]) for _ in range(count)] for _ in range(rows)], dtype=np.uint32)
        noise = np.array([[rng.choice([0, 5, 9, 10, 11, 2**64 - 1]) for _ in range(count)] for _ in range(rows)], dtype=np.uint64)
        if rows > 1:
            status[:, 0], noise[:, 0] = 0, 0                             # one column that stays valid
        for st, nz in ((status, noise), (status, None), (None, noise)):
            for bits, bound in ((0xFFFFFFFF, 10), (2, 2**64 - 1), (5, 9)):
                want = mask_ref(st, nz, bits, bound)
                got, num = P.shamir_valid_mask(st, nz, status_bits=bits, noise_bound=bound, params=p)
                assert got.tolist() == want and num == sum(want), (rows, count, bits, bound)
                # the [count][rows] layout read with strides (1, rows), into a marked buffer
                d_st = None if st is None else dev(np.ascontiguousarray(st.T).view(np.int32))
                d_nz = None if nz is None else dev(np.ascontiguousarray(nz.T))
                out = torch.full((count + 64,), 7, dtype=torch.uint8, device=DEV)
                n2 = torch.full((1,), -1, dtype=torch.int32, device=DEV)
                torch.cuda.synchronize()
                rc = lib.pvw_shamir_valid_mask_device(p._h, ptr(d_st), ptr(d_nz), bits, bound, count, rows, 1, rows, C.c_void_p(out.data_ptr() + 32),
                                                      ptr(n2), cur())
                assert rc == 0, _ffi.last_error(lib)
                torch.cuda.synchronize()
                o = out.cpu().numpy()
                assert o[32:32 + count].tolist() == want and (o[:32] == 7).all() and (o[32 + count:] == 7).all() and n2.item() == sum(want)
    # device tensors in place through the api
    st = torch.tensor([[0, 3, 0, 0, 1, 0]], dtype=torch.int32, device=DEV)
    dvm, dn = P.shamir_valid_mask(st, params=p)
    torch.cuda.synchronize()
    assert dvm.cpu().tolist() == [1, 0, 1, 1, 0, 1] and dn.item() == 4
    print("mask ok", flush=True)


def lagrange_rows(pm, idx, valid, targets):
    """uncentred residues [T][D] as Python integers"""
    return [[w % pm for w in row] for row in weights_ref(pm, idx, valid, targets)]


class NarrowHandover:
    """An old sharing over p = 2^61 - 1 whose D = 6 holders re-deal their shares (deal_party_shares, new degree 2) to n new parties;
    holder 1 is masked out.  pack = 1: a degree-2 sharing of one secret at the point 0; pack = 3: a packed sharing (degree 4) of
    three secrets at the points 0, -1, -2.  truth(valid)[j][m] = sum_d lambda_{d,m} f_d(j + 1) mod p from pvw_shamir_shares_host."""
    IDX, VALID, DEGREE = [0, 5, 2, 7, 3, 9], [1, 0, 1, 1, 1, 1], 2

    def __init__(self, n, pack=1, tag=0, system_=None, wrong=None):
        self.p, self.gpk, self.parties = system_ or system(M.bench_moduli(17), n, 16, 8)
        self.n, self.pm, self.pack = n, PLAIN, pack
        pm, D = self.pm, len(self.IDX)
        rnd = random.Random(1000 * n + 10 * pack + tag)
        self.secrets = [rnd.randrange(pm) for _ in range(pack)]
        old = _params(10)
        if pack == 1:
            y = P.shamir_shares(old, self.secrets, 2, pm, seeds=[bytes([tag + 1]) * 32], host=True)[0].tolist()
            self.targets = None
        else:
            y = P.shamir_shares_packed(old, [self.secrets], 2, pm, seeds=[bytes([tag + 1]) * 32], host=True)[0].tolist()
            self.targets = [pm - 1 - m for m in range(pack)]
        self.old_shares = [y[i] for i in self.IDX]
        if wrong is not None:
            self.old_shares[wrong] = (self.old_shares[wrong] + 12345) % pm
        seeds = [api._dealer_seed(bytes([0x2C]) * 32, 100 * tag + d) for d in range(D)]
        self.cts = P.deal_party_shares(self.old_shares, self.DEGREE, pm, self.gpk, seeds=seeds)
        self.shares = P.shamir_shares(self.p, self.old_shares, self.DEGREE, pm, seeds=seeds, host=True).tolist()      # [D][n]
        self.c1s, self.c2s = np.stack([c.c1 for c in self.cts]), np.stack([c.c2 for c in self.cts])
        self.T = 1 if self.targets is None else len(self.targets)

    def truth(self, valid=None):
        valid = self.VALID if valid is None else valid
        lam = lagrange_rows(self.pm, self.IDX, valid, self.targets)
        return [[sum(a * self.shares[d][j] for d, a in enumerate(row)) % self.pm for row in lam] for j in range(self.n)]

    def composition(self, lo, hi, valid=None, repr_=P.REPR_NTT, c1s=None, c2s=None):
        """pvw_shamir_handover_weights_host -> pvw_decrypt_all_lincomb_many_plain with the same arguments: (out, noise, status)"""
        p, D, NP, T = self.p, len(self.IDX), hi - lo, self.T
        valid = self.VALID if valid is None else valid
        rows, _ = P.shamir_handover_weights(None, self.IDX, self.pm, valid, self.targets, host=True)
        out, nz, st = np.zeros((NP, T), np.uint64), np.zeros((NP, T), np.uint64), np.zeros((NP, T), np.uint32)
        sk = np.ascontiguousarray(np.stack([pt.secret_key.secret_coeffs for pt in self.parties[lo:hi]]).astype(np.int64))
        c1s, c2s = (self.c1s if c1s is None else c1s), (self.c2s if c2s is None else c2s)
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        p._call("pvw_decrypt_all_lincomb_many_plain", lo, hi, api._ptr(sk), api._ptr(c1s), api._ptr(c2s), D, api._ptr(v), api._ptr(rows), T,
                repr_, api._ptr(out), api._ptr(nz), api._ptr(st), None, self.pm, 0, None)
        return out, nz, st

    def device_buffers(self, lo, hi, valid=None, c1s=None, c2s=None):
        sk = np.stack([pt.secret_key.secret_coeffs for pt in self.parties[lo:hi]]).astype(np.int64)
        valid = self.VALID if valid is None else valid
        return {"sk": dev(sk), "c1": dev(self.c1s if c1s is None else c1s), "c2": dev(self.c2s if c2s is None else c2s),
                "valid": torch.tensor(valid, dtype=torch.uint8, device=DEV),
                "out": torch.full((hi - lo, self.T), -1, dtype=torch.int64, device=DEV),
                "nz": torch.full((hi - lo, self.T), -1, dtype=torch.int64, device=DEV),
                "st": torch.full((hi - lo, self.T), -1, dtype=torch.int32, device=DEV), "cnt": torch.full((1,), -1, dtype=torch.int32, device=DEV)}

    def device(self, lo, hi, bufs, repr_=P.REPR_NTT, stream=None, indices=None):
        """pvw_decrypt_all_handover_device on buffers made by device_buffers: rc and the message"""
        lib = _ffi.lib()
        ix = np.array(self.IDX if indices is None else indices, dtype=np.uint64)
        tg = None if self.targets is None else np.array(self.targets, dtype=np.uint64)
        rc = lib.pvw_decrypt_all_handover_device(self.p._h, lo, hi, ptr(bufs["sk"]), ptr(bufs["c1"]), ptr(bufs["c2"]), len(self.IDX),
                                                 ptr(bufs["valid"]), api._ptr(ix), api._ptr(tg), self.T, repr_, ptr(bufs["out"]), ptr(bufs["nz"]),
                                                 ptr(bufs["st"]), ptr(bufs["cnt"]), self.pm, 0, None, stream or cur())
        return rc, _ffi.last_error(lib)

    def same(self, bufs, want):
        out, nz, st = want
        return (np.array_equal(u64(bufs["out"]), out) and np.array_equal(u64(bufs["nz"]), nz)
                and np.array_equal(bufs["st"].cpu().numpy().view(np.uint32), st))


def handover():
    """n = 12 (per-party path) and n = 24 (GEMM path), a plain and a packed old sharing: the one call gives the Python truth, equals
    the composition bit for bit (values, noise, status), t + 1 new shares reconstruct the old secrets; both representations, a
    sub-range of parties, both forms; the masked holder's ciphertext filled with arbitrary words changes nothing"""
    for n in (12, 24):
        for pack in (1, 3):
            h = NarrowHandover(n, pack)
            p, pm = h.p, h.pm
            rnd = random.Random(n + pack)
            truth = h.truth()
            rep = P.decrypt_all_party_handover(h.cts, h.parties, h.IDX, pm, h.VALID, h.targets)
            assert rep.values.tolist() == truth and rep.count == 5, (n, pack)
            comp = h.composition(0, n)
            assert np.array_equal(rep.residues, comp[0]) and np.array_equal(rep.noise, comp[1]) and np.array_equal(rep.status, comp[2])
            assert api._secret_residue(p)[0] == 0
            for m in range(pack):
                for _ in range(3):
                    who = rnd.sample(range(n), h.DEGREE + 1)
                    assert P.shamir_reconstruct(who, [truth[j][m] for j in who], pm) == h.secrets[m], (n, pack, m)
            # the api with the mask as a device tensor: the device form
            rep2 = P.decrypt_all_party_handover(h.cts, h.parties, h.IDX, pm, torch.tensor(h.VALID, dtype=torch.uint8, device=DEV), h.targets)
            assert rep2.values.tolist() == truth and rep2.count == 5 and np.array_equal(rep2.noise, comp[1])
            # POWER-basis input and a sub-range of parties, host buffers
            pw = [P.PvwCiphertext(p.ntt_inverse(c.c1), p.ntt_inverse(c.c2), p, P.REPR_POWER) for c in h.cts]
            lo, cnt = 1, 4
            rep3 = P.decrypt_all_party_handover(pw, h.parties[lo:lo + cnt], h.IDX, pm, h.VALID, h.targets)
            assert rep3.values.tolist() == truth[lo:lo + cnt], (n, pack)
            # device pointers, both representations; the masked holder's ciphertext is arbitrary words
            junk = np.random.default_rng(n).integers(0, 1 << 63, h.c1s[1].size + h.c2s[1].size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            for repr_, c1s, c2s in ((P.REPR_NTT, h.c1s.copy(), h.c2s.copy()),
                                    (P.REPR_POWER, np.stack([c.c1 for c in pw]), np.stack([c.c2 for c in pw]))):
                for lo, hi in ((0, n), (2, 7)):
                    want = h.composition(lo, hi, None, repr_, c1s, c2s)
                    assert want[0].tolist() == truth[lo:hi]
                    for spoil in (False, True):
                        if spoil:
                            c1s[1] = junk[:h.c1s[1].size].reshape(h.c1s[1].shape)
                            c2s[1] = junk[h.c1s[1].size:].reshape(h.c2s[1].shape)
                        bufs = h.device_buffers(lo, hi, None, c1s, c2s)
                        torch.cuda.synchronize()
                        rc, msg = h.device(lo, hi, bufs, repr_)
                        assert rc == 0, msg
                        torch.cuda.synchronize()
                        assert h.same(bufs, want) and bufs["cnt"].item() == 5, (n, pack, repr_, lo, spoil)
                        assert api._secret_residue(p)[0] == 0
            print(f"handover n={n} pack={pack} ok", flush=True)
    # nobody valid: the device form gives zeros and count 0, the host-buffer form the mirrored call's code; T = 3 (the
    # many-combinations pass) and T = 1 (the single-combination pass with an all-zero weight row)
    for h in (h, NarrowHandover(12, 1, tag=5)):
        n = h.n
        bufs = h.device_buffers(0, n, [0] * 6)
        torch.cuda.synchronize()
        rc, msg = h.device(0, n, bufs)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert not bufs["out"].any() and bufs["cnt"].item() == 0, h.T
        try:
            P.decrypt_all_party_handover(h.cts, h.parties, h.IDX, h.pm, [0] * 6, h.targets)
            raise AssertionError("not refused")
        except P.PvwError as e:
            assert e.code == 17
    print("handover ok", flush=True)


MASKS = ([1, 0, 1, 1, 1, 1], [1, 1, 1, 0, 1, 1], [0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1])


def remask():
    """the same device call again and again with the mask bytes changed in device memory between: each result equals the
    composition for its mask, and the old secrets come back under every mask"""
    n = 12
    for pack in (1, 3):
        h = NarrowHandover(n, pack, tag=1)
        bufs = h.device_buffers(0, n)
        seen = []
        for valid in MASKS:
            bufs["valid"].copy_(torch.tensor(valid, dtype=torch.uint8, device=DEV))
            torch.cuda.synchronize()
            rc, msg = h.device(0, n, bufs)
            assert rc == 0, msg
            torch.cuda.synchronize()
            assert h.same(bufs, h.composition(0, n, valid)) and bufs["cnt"].item() == sum(valid), (pack, valid)
            vals = u64(bufs["out"]).tolist()
            assert vals == h.truth(valid)
            for m in range(pack):
                assert P.shamir_reconstruct([0, 4, 9], [vals[j][m] for j in (0, 4, 9)], h.pm) == h.secrets[m]
            seen.append(vals)
        assert seen[0] != seen[1]                                       # other holders, other new shares of the same secret
    print("remask ok", flush=True)


def capture():
    """the device form is refused under capture on a stream nothing has sized, with nothing enqueued; after a call outside capture
    it is captured once and replayed with the mask changed on the device between the replays: every replay equals the composition
    for the mask of the moment.  T = 3 (the many-combinations pass) and T = 1 (the single-combination pass)."""
    n = 12
    sysm = system(M.bench_moduli(17), n, 16, 8)
    for pack in (3, 1):
        h = NarrowHandover(n, pack, tag=4, system_=sysm)
        bufs = h.device_buffers(0, n)
        s = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            rc, msg = h.device(0, n, bufs)
        torch.cuda.synchronize()
        assert rc == 1 and "outside capture first" in msg, (rc, msg)
        g0.replay()
        torch.cuda.synchronize()
        assert (bufs["out"] == -1).all() and (bufs["st"] == -1).all() and (bufs["cnt"] == -1).all() and (bufs["nz"] == -1).all()
        del g0
        with torch.cuda.stream(s):
            rc, msg = h.device(0, n, bufs)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert h.same(bufs, h.composition(0, n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc, msg = h.device(0, n, bufs)
        assert rc == 0, msg
        for valid in MASKS[1:] + MASKS[:1]:
            bufs["valid"].copy_(torch.tensor(valid, dtype=torch.uint8, device=DEV))
            bufs["out"].fill_(-1)
            bufs["cnt"].fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert h.same(bufs, h.composition(0, n, valid)) and bufs["cnt"].item() == sum(valid), (pack, valid)
        del g
        assert api._secret_residue(h.p)[0] == 0
    print("capture ok", flush=True)


def chain():
    """pvw_shamir_reconstruct_corrected_device over the old sharing with one wrong column -> pvw_shamir_valid_mask_device on its
    d_col_err -> pvw_decrypt_all_handover_device, all on one stream with no host read in between: the mask names the wrong
    holder, and the new shares reconstruct the old secret although that holder re-dealt its wrong share"""
    n = 12
    lib = _ffi.lib()
    for wrong in (1, 4):
        h = NarrowHandover(n, 1, tag=6, wrong=wrong)
        p = h.p
        D = len(h.IDX)
        bufs = h.device_buffers(0, n, [1] * D)
        bufs["valid"].fill_(7)
        d_sh = dev(np.array([h.old_shares], dtype=np.uint64))
        d_sec = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        d_nerr = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        d_col = torch.full((D,), -1, dtype=torch.int32, device=DEV)
        ix = np.array(h.IDX, dtype=np.uint64)
        torch.cuda.synchronize()
        rc = lib.pvw_shamir_reconstruct_corrected_device(p._h, h.pm, 2, api._ptr(ix), D, ptr(d_sh), 1, D, 1, ptr(d_sec), ptr(d_nerr), ptr(d_col),
                                                         None, cur())
        assert rc == 0, _ffi.last_error(lib)
        rc = lib.pvw_shamir_valid_mask_device(p._h, ptr(d_col), None, 0xFFFFFFFF, 0, D, 1, D, 1, ptr(bufs["valid"]), None, cur())
        assert rc == 0, _ffi.last_error(lib)
        rc, msg = h.device(0, n, bufs)
        assert rc == 0, msg
        torch.cuda.synchronize()
        valid = [int(d != wrong) for d in range(D)]
        assert u64(d_sec).tolist() == h.secrets and bufs["valid"].cpu().tolist() == valid and bufs["cnt"].item() == D - 1
        assert h.same(bufs, h.composition(0, n, valid))
        vals = u64(bufs["out"]).tolist()
        for who in ([0, 1, 2], [3, 7, 11]):
            assert P.shamir_reconstruct(who, [vals[j][0] for j in who], h.pm) == h.secrets[0]
    print("chain ok", flush=True)


def hygiene():
    """pvw_selftest_secret_residue is 0 after a successful call of either form and after a refusal, which writes nothing"""
    for n in (12, 24):
        h = NarrowHandover(n, tag=2)
        p = h.p
        rep = P.decrypt_all_party_handover(h.cts, h.parties, h.IDX, h.pm, h.VALID)
        assert rep.values.tolist() == h.truth() and api._secret_residue(p)[0] == 0
        try:
            P.decrypt_all_party_handover(h.cts, h.parties, [0, 5, 2, 7, 3, 3], h.pm, h.VALID)     # a duplicate holder
            raise AssertionError("not refused")
        except P.PvwError as e:
            assert e.code == 1
        assert api._secret_residue(p)[0] == 0
        bufs = h.device_buffers(0, n)
        torch.cuda.synchronize()
        rc, msg = h.device(0, n, bufs)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert u64(bufs["out"]).tolist() == h.truth() and api._secret_residue(p)[0] == 0
        marked = {k_: v.clone() for k_, v in bufs.items()}
        rc, msg = h.device(0, n, bufs, indices=[0, 5, 2, 7, 3, 5])         # a duplicate although holder 1 is masked
        torch.cuda.synchronize()
        assert rc == 1 and all(torch.equal(bufs[k_], marked[k_]) for k_ in bufs) and api._secret_residue(p)[0] == 0
    print("hygiene ok", flush=True)


class group_budget:
    """PVW_EVALUATE_GROUP_BYTES around one call (None: unset)"""

    def __init__(self, b):
        self.b = b

    def __enter__(self):
        os.environ.pop("PVW_EVALUATE_GROUP_BYTES", None)
        if self.b is not None:
            os.environ["PVW_EVALUATE_GROUP_BYTES"] = str(self.b)

    def __exit__(self, *exc):
        os.environ.pop("PVW_EVALUATE_GROUP_BYTES", None)


def pieces():
    """the tuning build: PVW_EVALUATE_GROUP_BYTES so small that the weights walk their targets in several groups (65 targets ten at
    a time; the handover's three one at a time), and PVW_STAGE_BYTES so small that the many-combinations pass inside the
    host-buffer call stages its five valid holders in several pieces: the same words as in one piece"""
    _ffi.select("tuning")
    p = _params(3)
    rng = random.Random(7)
    D, T = 65, 65
    idx = indices_for(D, P62, rng)
    valid = [int(d % 3 != 1) for d in range(D)]
    targets = [P62 - 1, idx[0], idx[1]] + [rng.randrange(P62) for _ in range(T - 3)]
    want, wcount = P.shamir_handover_weights(None, idx, P62, valid, targets, host=True)
    for gb in (None, 10 * ((D + 2) * 8 + 4), (D + 2) * 8 + 4, 1):
        with group_budget(gb):
            got, count, intact = device_weights(p, idx, P62, valid, targets)
        assert intact and count == wcount and np.array_equal(got, want), gb
    n = 12
    h = NarrowHandover(n, 3, tag=3)
    item = (h.p.k + n) * h.p.L * h.p.l * 8
    truth = h.truth()
    for bb, gb in ((None, None), (2 * item + item // 2, (6 + 2) * 8 + 4), (item + item // 2, 1)):
        with budget(bb), group_budget(gb):
            rep = P.decrypt_all_party_handover(h.cts, h.parties, h.IDX, h.pm, h.VALID, h.targets)
            bufs = h.device_buffers(0, n)
            torch.cuda.synchronize()
            rc, msg = h.device(0, n, bufs)
            assert rc == 0, msg
            torch.cuda.synchronize()
        assert rep.values.tolist() == truth and rep.count == 5 and u64(bufs["out"]).tolist() == truth, (bb, gb)
        assert api._secret_residue(h.p)[0] == 0
    _ffi.select("default")
    print("pieces ok", flush=True)


def threads():
    """two threads on one context call the host-buffer form next to each other (two masks, all parties and a sub-range): every
    result is the serial twin's"""
    n = 12
    h = NarrowHandover(n, 3, tag=8)
    p = h.p

    def job(valid, lo, hi):
        rep = P.decrypt_all_party_handover(h.cts, h.parties[lo:hi], h.IDX, h.pm, valid, h.targets)
        return rep.values.tolist(), rep.noise.tolist(), rep.status.tolist(), rep.count

    plans = [[(MASKS[0], 0, n), (MASKS[1], 2, 7), (MASKS[0], 0, n)], [(MASKS[2], 0, n), (MASKS[0], 0, n), (MASKS[3], 1, 5)]]
    serial = [[job(*a) for a in plan] for plan in plans]
    assert serial[0][0][0] == h.truth() and serial[1][2][0] == h.truth(MASKS[3])[1:5]
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


CASES = {f.__name__: f for f in (weights, mask, handover, remask, capture, chain, hygiene, pieces, threads)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("SHAMIR_HANDOVER_OK")

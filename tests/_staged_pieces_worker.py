"""Every host-buffer entry point of pvw_capi.hip taken through SEVERAL staged pieces at small shapes: the tuning build with a small
PVW_STAGE_BYTES against (a) an independent reference -- pvw_ct_sum_host, pvw_shamir_shares_host, the host decodes
of single-ciphertext noisy polynomials, the dealt plaintexts, single-dealer pvw_encrypt calls -- and (b) the same call in one
piece with the default budget.  Bit for bit.  Each case restates the library's piece arithmetic in Python and asserts the
split it claims, so no case can quietly run in one piece.  torch is imported FIRST so both libraries share one HIP runtime.
Spawned case by case by tests/test_gpu_staged_pieces.py; prints STAGED_PIECES_OK."""
import ctypes as C
import os
import sys
import time

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
from test_ct_sum_host import _words  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
S = bytes(range(101, 133))          # the randomness state's seed
U64 = (1 << 64) - 1
GIB = 1 << 30
PM = (1 << 61) - 1
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)
ptr = api._ptr
GEOMS = (("3x61", M.bench_moduli(3)), ("4x56", EXAMPLE_MODULI))   # 4x56: the 7-byte contraction of the digit GEMM


# ---- the library's piece arithmetic, restated ------------------------------------------------------------------------------
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


def chunk(item_bytes, most, b=GIB):
    per = b // item_bytes
    return 1 if per == 0 else min(per, most)


def cut(D, per):
    return [min(per, D - d0) for d0 in range(0, D, per)]


def passes(item_bytes, D, b=GIB):
    """encrypt_multi_stage (pvw_encrypt_multi*, pvw_deal_shares*): half the budget, at least 4 dealers, a multiple of 4"""
    per = max((b // 2) // item_bytes, 4) & ~3
    return cut(D, min(per, D))


def sum_fills(D, valid, per):
    """ct_sum_staged: the dealers summed by each launch"""
    fills, fill, d = [], 0, 0
    while d < D:
        if valid is not None and not valid[d]:
            d += 1
            continue
        run = 1
        while d + run < D and fill + run < per and (valid is None or valid[d + run]):
            run += 1
        fill, d = fill + run, d + run
        if fill == per:
            fills.append(fill)
            fill = 0
    return fills + ([fill] if fill else [])


def sum_slices(items, dealers):
    """ct_sum_slices and the cap of ct_sum_enqueue"""
    wgs = (items + 255) // 256
    ns = min(1 if wgs >= 512 else (1024 + wgs - 1) // wgs, 64)
    while ns > 1 and dealers // ns < 8:
        ns -= 1
    return min(ns, 1536 * 256 // items)


def all_layout(p, NP, D, host, stage, b=GIB):
    """decrypt_all_layout: (party by party) Dc, or (matrix cores) Dg and Pc"""
    Pw = p.L * p.l
    ctw = p.k * Pw
    if NP < 22:
        return {"gemm": False, "Dc": chunk(ctw * 8, D, b)}
    Dg = min(D, 128)
    while Dg > 1 and Dg * ctw * 72 > b:
        Dg //= 2
    nbg = (Dg + 15) // 16
    per_party = ctw * 8 * (1 if p.l <= 32 else 2) + nbg * 16 * Pw * 8 + Dg * Pw * 8 * (2 if stage else 1) + Dg * 8 + (p.k * p.l * 8 if host else 0)
    Pc = 3 * b // per_party
    if Pc >= NP:
        Pc = NP
    elif Pc >= 128:
        Pc -= Pc % 128
    return {"gemm": True, "Dg": Dg, "Pc": max(Pc, 1)}


def find_budget(p, NP, D, host, stage, want):
    for b in range(8 << 20, 4096, -4096):
        if want(all_layout(p, NP, D, host, stage, b)):
            return b
    raise AssertionError("no budget gives the layout asked for")


# ---- systems ---------------------------------------------------------------------------------------------------------------
def params(n, k, l, moduli, shard=None):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if shard:
        b = b.set_shard(*shard)
    return b.build()


def system(moduli, n, k=32, l=8, shard=None, keys=True):
    p = params(n, k, l, moduli, shard)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = None
    if keys:
        parties = [P.Party.new(i, p, SEED) for i in range(n)]
        gpk.generate_all_party_keys(parties, SEED)
    else:
        gpk.fill_uniform(SEED)
    return p, gpk, parties


def dealt(p, gpk, shares, tag, repr=P.REPR_NTT):
    """one-pass pvw_encrypt_multi (default budget) of shares [D][n]: c1s [D][k][L][l], c2s [D][n][L][l]"""
    with budget(None):
        cts = P.encrypt_many(shares.tolist(), gpk, [api._dealer_seed(SEED, tag + d) for d in range(len(shares))], repr)
    return np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts])


def clean(p, what):
    assert api._secret_residue(p)[0] == 0, ("key material left on the device", what)


def noisy_of(p, c1, c2row, sk):
    """the noisy polynomial of ONE ciphertext (one piece whatever the budget): [L][l]"""
    out, nz = np.zeros(1, np.uint64), np.zeros((1, p.L, p.l), np.uint64)
    with budget(None):
        p._call("pvw_decrypt_batch", ptr(sk), ptr(np.ascontiguousarray(c1[None])), ptr(np.ascontiguousarray(c2row[None])), 1, P.REPR_NTT,
                ptr(out), ptr(nz))
    return nz[0]


def host_decode(p, nz, plain_modulus=0, ww=0):
    """pvw_decode_checked_host, or pvw_decode_plain_host with a modulus / wide words: (out, noise, status, wide)"""
    a = np.ascontiguousarray(nz).reshape(-1, p.L, p.l)
    out, noise, status = np.zeros(len(a), np.uint64), np.zeros(len(a), np.uint64), np.zeros(len(a), np.uint32)
    wide = np.zeros((len(a), ww), np.uint64)
    if plain_modulus or ww:
        p._call("pvw_decode_plain_host", ptr(a), len(a), ptr(out), ptr(noise), ptr(status), plain_modulus, ww, ptr(wide) if ww else None)
    else:
        p._call("pvw_decode_checked_host", ptr(a), len(a), ptr(out), ptr(noise), ptr(status))
    return out, noise, status, wide


def tamper(p, poly):
    """one residue of an [L][l] polynomial replaced"""
    poly[1, 2] = np.uint64((int(poly[1, 2]) + 12345) % int(p.moduli()[1]))


# ---- sum ---------------------------------------------------------------------------------------------------------------------
def run_sum(p, c1s, c2s, valid, lo, hi, b):
    c1, c2 = np.full((p.k, p.L, p.l), MARK), np.full((hi - lo, p.L, p.l), MARK)
    cnt = C.c_uint32(77)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    with budget(b):
        p._call("pvw_ct_sum", ptr(c1s), ptr(c2s), len(c1s), ptr(v), lo, hi, ptr(c1), ptr(c2), C.byref(cnt))
    return c1, c2, cnt.value


def case_sum():
    """pvw_ct_sum: D = 7 at pieces of 1, 2, 3 (the unsplit kernel accumulating) and D = 40 at pieces of 16 (two slices each:
    ct_sum_finish accumulating, then an unsplit accumulating tail), any / extreme words, masks, row ranges, the count"""
    n, k, l = 40, 32, 8
    p = params(n, k, l, M.bench_moduli(3))
    Pw = p.L * l
    for D, pers in ((7, (1, 2, 3)), (40, (16,))):
        masks = {"none": None, "alternating": np.arange(D) % 2 == 0, "straddle": ~np.isin(np.arange(D), (2, 5)), "one": np.arange(D) == D // 2}
        for kind in ("any", "extreme"):
            rng = np.random.default_rng(D + len(kind))
            c1s, c2s = _words(rng, p, D, k, kind), _words(rng, p, D, n, kind)
            for lo, hi in ((0, n), (1, n), (n - 1, n)):
                item = (k + hi - lo) * Pw * 8
                for mname, valid in masks.items():
                    nv = D if valid is None else int(valid.sum())
                    w1, w2 = np.zeros((k, p.L, l), np.uint64), np.zeros((hi - lo, p.L, l), np.uint64)
                    v8 = None if valid is None else valid.astype(np.uint8)
                    p._call("pvw_ct_sum_host", ptr(c1s), ptr(c2s), D, ptr(v8), lo, hi, ptr(w1), ptr(w2), None)
                    assert sum_fills(D, valid, chunk(item, nv)) == [nv]
                    o1, o2, oc = run_sum(p, c1s, c2s, valid, lo, hi, None)                       # (b): one piece
                    assert np.array_equal(o1, w1) and np.array_equal(o2, w2) and oc == nv, ("one piece", D, kind, lo, hi, mname)
                    for per in pers:
                        b = per * item + item // 2
                        fills = sum_fills(D, valid, chunk(item, nv, b))
                        what = (D, kind, lo, hi, mname, per, fills)
                        if mname == "one":
                            assert fills == [1], what              # one valid dealer is one piece by necessity: the skipping is the point
                        else:
                            assert len(fills) >= 2 and max(fills) == per, what
                        if mname == "none":
                            assert fills == cut(D, per), what
                            if (D, per) == (7, 3):
                                assert fills == [3, 3, 1]
                            if D == 40:
                                assert fills == [16, 16, 8] and [sum_slices(item // 16, f) for f in fills] == [2, 2, 1], what
                        if (mname, per) == ("straddle", 3):
                            assert fills == [3, 2], what           # dealers 0 1 | 3, then 4 | 6: runs cut by the mask and by the piece
                        g1, g2, gc = run_sum(p, c1s, c2s, valid, lo, hi, b)
                        assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and gc == nv, what
                    print(f"sum D={D} {kind} rows [{lo},{hi}) mask {mname}: pieces", [sum_fills(D, valid, chunk(item, nv, q * item + item // 2)) for q in pers],
                          flush=True)


# ---- sum_decrypt -----------------------------------------------------------------------------------------------------------
def triple(r):
    return [(int(a), int(b), int(c)) for a, b, c in zip(r.residues, r.noise, r.status)]


def case_sum_decrypt():
    """decrypt_party_sum and decrypt_all_party_sums (5 parties; all n: both sides of the 22-party dispatch), D = 24 in pieces
    of 5, NTT and POWER input, with and without plain_modulus = 2^61 - 1: the sum of the dealt shares and the host decode of
    the noisy polynomial of the host-summed ciphertext"""
    n, k, l, D, per = 40, 32, 8, 24, 5
    for name, moduli in GEOMS:
        p, gpk, parties = system(moduli, n, k, l)
        Pw = p.L * l
        # pvw_ctx_sum_capacity is a sufficient radius (17 dealers at 3 x 61 bits, 433 at 4 x 56): exactness is asserted, not assumed
        assert name != "4x56" or p.sum_capacity() >= D
        shares = np.random.default_rng(7).integers(0, 1 << 57, (D, n), dtype=np.uint64)
        c1s, c2s = dealt(p, gpk, shares, 0)
        want = [int(shares[:, i].astype(object).sum()) for i in range(n)]
        a1, a2 = np.zeros((k, p.L, l), np.uint64), np.zeros((n, p.L, l), np.uint64)
        p._call("pvw_ct_sum_host", ptr(c1s), ptr(c2s), D, None, 0, n, ptr(a1), ptr(a2), None)
        nz = np.stack([noisy_of(p, a1, a2[i], api._i64(parties[i].secret_key.secret_coeffs)) for i in range(n)])
        clean(p, name)
        refs = {None: host_decode(p, nz), PM: host_decode(p, nz, PM)}
        for i in range(n):
            assert int(refs[None][0][i]) == want[i] and int(refs[None][2][i]) == 0 and int(refs[PM][0][i]) == want[i] % PM, (name, i)
        ref = lambda pm, i: (int(refs[pm][0][i]), int(refs[pm][1][i]), int(refs[pm][2][i]))
        for repr in (P.REPR_NTT, P.REPR_POWER):
            if repr == P.REPR_POWER:
                with budget(None):
                    c1s, c2s = p.ntt_inverse(c1s), p.ntt_inverse(c2s)
            cts = [P.PvwCiphertext(c1s[d], c2s[d], p, repr) for d in range(D)]
            for pm in (None, PM):
                for i in (0, 17, n - 1):
                    item = (k + 1) * Pw * 8
                    assert sum_fills(D, None, chunk(item, D)) == [D] and sum_fills(D, None, chunk(item, D, per * item)) == [5, 5, 5, 5, 4]
                    for b in (None, per * item):
                        with budget(b):
                            r = P.decrypt_party_sum(cts, parties[i].secret_key, i, plain_modulus=pm)
                        assert triple(r) == [ref(pm, i)], (name, repr, pm, i, b)
                        clean(p, (name, "party sum", b))
                for lo, cnt in ((3, 5), (0, n)):
                    item = (k + cnt) * Pw * 8
                    assert sum_fills(D, None, chunk(item, D)) == [D] and sum_fills(D, None, chunk(item, D, per * item)) == [5, 5, 5, 5, 4]
                    for b in (None, per * item):
                        with budget(b):
                            r = P.decrypt_all_party_sums(cts, parties[lo:lo + cnt], plain_modulus=pm)
                        assert triple(r) == [ref(pm, lo + j) for j in range(cnt)], (name, repr, pm, lo, cnt, b)
                        clean(p, (name, "all sums", b))
            print(f"sum_decrypt {name} repr {repr}: pieces [5, 5, 5, 5, 4] for 1, 5 and {n} parties, with and without a plain modulus", flush=True)


# ---- batch -----------------------------------------------------------------------------------------------------------------
def run_batch(p, sk, c1s, col, repr, form, b):
    D = len(c1s)
    o = {"out": np.full(D, MARK), "noisy": np.full((D, p.L, p.l), MARK), "noise": np.full(D, MARK),
         "status": np.full(D, 0xA5A5A5A5, np.uint32), "wide": np.full((D, 3), MARK)}
    head = (ptr(sk), ptr(c1s), ptr(col), D, repr, ptr(o["out"]))
    with budget(b):
        if form == "values":
            p._call("pvw_decrypt_batch", *head, ptr(o["noisy"]))
        elif form == "checked":
            p._call("pvw_decrypt_batch_checked", *head, ptr(o["noise"]), ptr(o["status"]))
        else:
            p._call("pvw_decrypt_batch_plain", *head, ptr(o["noise"]), ptr(o["status"]), PM, 3, ptr(o["wide"]))
    clean(p, ("batch", form, b))
    return o


def case_batch():
    """pvw_decrypt_batch (noisy_out requested), _checked and _plain (2^61 - 1, three wide words), NTT and POWER input: D = 7 at
    pieces of 1 and 3, D = 130 at pieces of 64; shares from 2^63 up (negative as the encoder reads them: the wide words carry
    |P|); one tampered ciphertext in the second piece shows at its own index only"""
    n, k, l, i = 40, 32, 8, 3
    for name, moduli in GEOMS:
        p, gpk, parties = system(moduli, n, k, l)
        sk = api._i64(parties[i].secret_key.secret_coeffs)
        item, bound = k * p.L * l * 8, p.noise_bound()
        for D, pers in ((7, (1, 3)), (130, (64,))):
            shares = np.random.default_rng(D).integers(0, 1 << 63, (D, n), dtype=np.uint64)
            shares[::3] |= np.uint64(1 << 63)
            c1s, c2s = dealt(p, gpk, shares, 1000)
            col = np.ascontiguousarray(c2s[:, i])
            nz_clean = np.stack([noisy_of(p, c1s[d], col[d], sk) for d in range(D)])
            for per in pers:
                bad = per + (per > 1)                                   # in the second piece, not at its first index unless per = 1
                b = per * item + item // 2
                assert cut(D, chunk(item, D)) == [D] and cut(D, chunk(item, D, b)) == cut(D, per) and D > per and bad // per == 1
                colb = col.copy()
                tamper(p, colb[bad])
                nz = nz_clean.copy()
                nz[bad] = noisy_of(p, c1s[bad], colb[bad], sk)
                rc, rp = host_decode(p, nz), host_decode(p, nz, PM, 3)
                for d in range(D):
                    s = int(shares[d][i])
                    if d == bad:                                        # flagged by the references themselves
                        assert int(rc[2][d]) != 0 or int(rc[1][d]) > bound, (name, D, per)
                        continue
                    assert int(rc[1][d]) <= bound and int(rp[1][d]) <= bound, (name, D, d)
                    if s < 1 << 63:
                        assert (int(rc[0][d]), int(rc[2][d]), int(rp[0][d]), int(rp[2][d])) == (s, 0, s % PM, 0), (name, D, d)
                        assert [int(x) for x in rp[3][d]] == [s, 0, 0], (name, D, d)
                    else:
                        assert int(rp[0][d]) == (s - (1 << 64)) % PM and int(rp[2][d]) & api.DEC_NEGATIVE, (name, D, d)
                        assert [int(x) for x in rp[3][d]] == [(1 << 64) - s, 0, 0], (name, D, d)
                with budget(None):
                    pw1, pw2 = p.ntt_inverse(c1s), p.ntt_inverse(colb)
                for repr, x1, x2 in ((P.REPR_NTT, c1s, colb), (P.REPR_POWER, pw1, pw2)):
                    for form, fields, r in (("values", ("out", "noisy"), (rc[0], nz)), ("checked", ("out", "noise", "status"), rc[:3]),
                                            ("plain", ("out", "noise", "status", "wide"), rp)):
                        for bb in (None, b):
                            o = run_batch(p, sk, x1, x2, repr, form, bb)
                            for f, w in zip(fields, r):
                                diff = np.nonzero((o[f] != w).reshape(D, -1).any(axis=1))[0]
                                assert diff.size == 0, (name, D, per, repr, form, bb, f, "items that differ", diff.tolist())
                print(f"batch {name} D={D}: pieces {cut(D, per)}, tampered ciphertext {bad}", flush=True)


# ---- all -------------------------------------------------------------------------------------------------------------------
def run_all(p, lo, sk, c1s, c2s, repr, form, b, device=False):
    NP, D = len(sk), len(c1s)
    shape = (NP, D)
    o = {"out": np.full(shape, MARK), "noise": np.full(shape, MARK), "status": np.full(shape, 0xA5A5A5A5, np.uint32),
         "wide": np.full(shape + (3,), MARK)}
    if device:
        t = {f: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(DEV) for f, a in o.items()}
        d_sk, d1, d2 = torch.from_numpy(sk).to(DEV), torch.from_numpy(c1s.view(np.int64)).to(DEV), torch.from_numpy(c2s.view(np.int64)).to(DEV)
        dp = lambda x: C.c_void_p(x.data_ptr())
        torch.cuda.synchronize()
        with budget(b):
            p._call("pvw_decrypt_all_plain_device", lo, lo + NP, dp(d_sk), dp(d1), dp(d2), D, repr, dp(t["out"]), dp(t["noise"]), dp(t["status"]),
                    PM, 3, dp(t["wide"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        o = {f: x.cpu().numpy().view(o[f].dtype) for f, x in t.items()}
    else:
        head = (lo, lo + NP, ptr(sk), ptr(c1s), ptr(c2s), D, repr, ptr(o["out"]))
        with budget(b):
            if form == "values":
                p._call("pvw_decrypt_all", *head)
            elif form == "checked":
                p._call("pvw_decrypt_all_checked", *head, ptr(o["noise"]), ptr(o["status"]))
            else:
                p._call("pvw_decrypt_all_plain", *head, ptr(o["noise"]), ptr(o["status"]), PM, 3, ptr(o["wide"]))
    clean(p, ("all", form, b, device))
    return o


def all_one(name, p, gpk, parties, lo, NP, D, bad, layouts):
    """layouts: {label: predicate on all_layout}; bad: (party, dealer) relative to lo, tampered"""
    n, k, l = p.n, p.k, p.l
    shares = np.random.default_rng(NP + D).integers(0, 1 << 57, (D, n), dtype=np.uint64)
    c1s, c2s = dealt(p, gpk, shares, 2000)
    tamper(p, c2s[bad[1], lo + bad[0]])
    sk = np.ascontiguousarray(np.stack([api._i64(pt.secret_key.secret_coeffs) for pt in parties[lo:lo + NP]]))
    # references: the dealt values everywhere but the tampered cell, whose report is the host decode of its own noisy polynomial
    want = np.ascontiguousarray(shares[:, lo:lo + NP].T)
    nzb = noisy_of(p, c1s[bad[1]], c2s[bad[1], lo + bad[0]], sk[bad[0]])
    rc, rp = host_decode(p, nzb), host_decode(p, nzb, PM, 3)
    bound = p.noise_bound()
    assert int(rc[2][0]) != 0 or int(rc[1][0]) > bound
    with budget(None):
        pw1, pw2 = p.ntt_inverse(c1s), p.ntt_inverse(c2s)

    def check(o, form, what):
        w = {"values": want, "checked": want, "plain": want % np.uint64(PM)}[form].copy()
        w[bad] = (rp if form == "plain" else rc)[0][0]
        cells = np.argwhere(o["out"] != w)
        assert cells.size == 0, (what, "cells [party, dealer] whose value differs", cells[:20].tolist())
        if form == "values":
            return
        ref = rp if form == "plain" else rc
        flagged = (o["status"] != 0) | (o["noise"] > np.uint64(bound))
        assert np.argwhere(flagged).tolist() == [list(bad)], (what, "flagged cells", np.argwhere(flagged)[:20].tolist())
        assert (int(o["noise"][bad]), int(o["status"][bad])) == (int(ref[1][0]), int(ref[2][0])), what
        if form == "plain":
            ww = np.zeros((NP, D, 3), np.uint64)
            ww[..., 0] = want
            ww[bad] = rp[3][0]
            cells = np.argwhere((o["wide"] != ww).any(axis=2))
            assert cells.size == 0, (what, "cells whose wide words differ", cells[:20].tolist())

    for label, pred in layouts.items():
        for device in (False, True):
            host = not device
            one = all_layout(p, NP, D, host, True)
            assert one == ({"gemm": True, "Dg": D, "Pc": NP} if NP >= 22 else {"gemm": False, "Dc": D})
            b = find_budget(p, NP, D, host, True, pred)
            lay = all_layout(p, NP, D, host, True, b)
            for bb in (None, b):
                if device:
                    check(run_all(p, lo, sk, pw1, pw2, P.REPR_POWER, "plain", bb, True), "plain", (name, label, "device POWER", bb, lay))
                else:
                    for form in ("values", "checked", "plain"):
                        check(run_all(p, lo, sk, c1s, c2s, P.REPR_NTT, form, bb), form, (name, label, form, bb, lay))
            if lay["gemm"]:
                print(f"all {name} {label} {'device' if device else 'host'}: budget {b}, party chunks {cut(NP, lay['Pc'])}, dealer groups {cut(D, lay['Dg'])}", flush=True)
            else:
                print(f"all {name} {label} {'device' if device else 'host'}: budget {b}, dealer chunks {cut(D, lay['Dc'])}", flush=True)


def case_all():
    """pvw_decrypt_all, _checked, _plain with host buffers and pvw_decrypt_all_plain_device with POWER input: party by party
    (5 parties, D = 7, Dc = 3) and on the matrix cores (300 parties, D = 37: Pc = 128 in three chunks; Pc < 128 that does not
    divide 300; Dg halved to a value that does not divide 37), one tampered cell with p0 > 0 and d0 > 0"""
    for name, moduli in GEOMS:
        p, gpk, parties = system(moduli, 40)
        all_one(name, p, gpk, parties, 2, 5, 7, (3, 5), {"party by party Dc=3": lambda a: not a["gemm"] and a["Dc"] == 3})
        p, gpk, parties = system(moduli, 300)
        all_one(name, p, gpk, parties, 0, 300, 37, (297, 36), {
            "Pc=128": lambda a: a["Pc"] == 128 and a["Dg"] == 37,
            "Pc<128": lambda a: a["Pc"] < 128 and 300 % a["Pc"] != 0 and a["Pc"] >= 40,
            "Dg halved": lambda a: a["Dg"] == 4 and 300 % a["Pc"] != 0,
        })


# ---- encrypt ---------------------------------------------------------------------------------------------------------------
def single(p, gpk, scalars, seed, repr):
    with budget(None):
        ct = P.encrypt([int(x) for x in scalars], gpk, seed, repr=repr)
    return ct.c1, ct.c2


def case_encrypt():
    """pvw_encrypt_multi[_rs] and pvw_deal_shares[_rs] in passes of 4: D = 9 (4, 4, 1) and D = 6 (4, 2), the last pass on the
    VALU where the one-pass call took the matrix cores; NTT and POWER output; a sharded context; the counter afterwards"""
    n, k, l, t, c0 = 40, 32, 8, 7, 77
    shard = (13, 31, 4, 29)
    for name, moduli in GEOMS:
        full = system(moduli, n, k, l)
        part = system(moduli, n, k, l, shard, keys=False), system(moduli, n, k, l, None, keys=False)   # the shard and its unsharded twin
        for label, (p, gpk, _), (rp_, rgpk, _), sh in (("full", full, full, (0, n, 0, k)), ("shard", part[0], part[1], shard)):
            rA, rB = sh[3] - sh[2], sh[1] - sh[0]
            Pw = p.L * l
            for D in (9, 6):
                rng = np.random.default_rng(D)
                scalars = rng.integers(0, 1 << 63, (D, n), dtype=np.uint64)
                secrets = rng.integers(0, 1 << 64, D, dtype=np.uint64)
                seeds = [api._dealer_seed(SEED, 300 + d) for d in range(D)]
                rs_seeds = [P.DeviceRandomness.call_seed(S, c0 + d) for d in range(D)]
                split = {9: [4, 4, 1], 6: [4, 2]}[D]
                for repr in (P.REPR_NTT, P.REPR_POWER):
                    for deal in (False, True):
                        item = (rA + rB) * Pw * 8 + (8 if deal else n * 8)
                        b = 8 * item
                        assert passes(item, D) == [D] and passes(item, D, b) == split
                        for rs in (False, True):
                            sd = rs_seeds if rs else seeds
                            rows = scalars
                            if deal:
                                rows = P.shamir_shares(rp_, secrets.tolist(), t, PM, seeds=sd, host=True)
                            ref = [single(rp_, rgpk, rows[d], sd[d], repr) for d in range(D)]
                            for bb in (None, b):
                                c1, c2 = np.full((D, k, p.L, l), MARK), np.full((D, n, p.L, l), MARK)
                                sdb = np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()
                                if deal:
                                    # a one-dealer deal (VALU: it marks and clears the r-hat vectors, tests/_shamir_worker.py
                                    # hygiene) so that what the scan finds afterwards is what the deal under test left
                                    with budget(None):
                                        p._call("pvw_deal_shares", ptr(secrets), 1, 1, PM, ptr(sdb), ptr(c1), ptr(c2), repr)
                                    clean(p, "before the deal")
                                    c1[:], c2[:] = MARK, MARK
                                with P.DeviceRandomness(p, S, c0) as st, budget(bb):
                                    if deal and rs:
                                        p._call("pvw_deal_shares_rs", ptr(secrets), D, t, PM, st._h, ptr(c1), ptr(c2), repr)
                                    elif deal:
                                        p._call("pvw_deal_shares", ptr(secrets), D, t, PM, ptr(sdb), ptr(c1), ptr(c2), repr)
                                    elif rs:
                                        p._call("pvw_encrypt_multi_rs", ptr(scalars), D, n, st._h, ptr(c1), ptr(c2), repr)
                                    else:
                                        p._call("pvw_encrypt_multi", ptr(scalars), D, n, ptr(sdb), ptr(c1), ptr(c2), repr)
                                    assert st.counter() == c0 + (D if rs else 0), (name, label, D, deal, rs, bb)
                                what = (name, label, D, repr, "deal" if deal else "encrypt", "rs" if rs else "seeded", bb)
                                bad = [d for d in range(D) if not (np.array_equal(c1[d, sh[2]:sh[3]], ref[d][0][sh[2]:sh[3]]) and
                                                                   np.array_equal(c2[d, sh[0]:sh[1]], ref[d][1][sh[0]:sh[1]]))]
                                assert not bad, (what, "dealers that differ", bad)
                                keep = np.ones(k, bool), np.ones(n, bool)
                                keep[0][sh[2]:sh[3]] = False
                                keep[1][sh[0]:sh[1]] = False
                                assert (c1[:, keep[0]] == MARK).all() and (c2[:, keep[1]] == MARK).all(), (what, "rows outside the shard written")
                                if deal:
                                    clean(p, what)
                print(f"encrypt {name} {label} D={D}: passes {split} (one pass: [{D}]), multi / deal, seeded / rs, NTT / POWER", flush=True)


# ---- shamir ----------------------------------------------------------------------------------------------------------------
def case_shamir():
    """pvw_shamir_shares at D = 7 in pieces of 3: drawn and explicit coefficients (unreduced 64-bit words), and a sharded
    context, whose call leaves the columns outside [13, 31) untouched"""
    n, t, D, per = 40, 7, 7, 3
    full, part = params(n, 32, 8, M.bench_moduli(3)), params(n, 32, 8, M.bench_moduli(3), (13, 31, 0, 32))
    rng = np.random.default_rng(4)
    secrets = rng.integers(0, 1 << 64, D, dtype=np.uint64)
    seeds = [api._dealer_seed(SEED, 500 + d) for d in range(D)]
    sdb = np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()
    coeffs = rng.integers(0, 1 << 64, (D, t), dtype=np.uint64)
    coeffs[1] = U64
    for cname, co in (("drawn", None), ("explicit", coeffs)):
        item = (n + (t if co is not None else 0) + 1) * 8
        b = per * item + 4
        assert cut(D, chunk(item, D)) == [D] and cut(D, chunk(item, D, b)) == [3, 3, 1]
        want = np.zeros((D, n), np.uint64)
        full._call("pvw_shamir_shares_host", ptr(secrets), D, t, PM, ptr(sdb), ptr(co), ptr(want))
        for label, p, lo, hi in (("full", full, 0, n), ("shard", part, 13, 31)):
            for bb in (None, b):
                out = np.full((D, n), MARK)
                with budget(bb):
                    p._call("pvw_shamir_shares", ptr(secrets), D, t, PM, ptr(sdb), ptr(co), ptr(out))
                rows = np.nonzero((out[:, lo:hi] != want[:, lo:hi]).any(axis=1))[0]
                assert rows.size == 0, (cname, label, bb, "dealers that differ", rows.tolist())
                assert (out[:, :lo] == MARK).all() and (out[:, hi:] == MARK).all(), (cname, label, bb, "columns outside the shard written")
                clean(p, (cname, label, bb))
        print(f"shamir {cname}: pieces [3, 3, 1] (one piece: [{D}]), full and sharded", flush=True)


# ---- real_bound ------------------------------------------------------------------------------------------------------------
def case_real_bound():
    """the shipped library, no selector: pvw_ct_sum at k = 256, l = 8, 17 moduli, rows [0, 1), D = 3900 any words is 1.09 GB
    and takes two pieces of the constant itself"""
    _ffi.select("default")
    os.environ["PVW_STAGE_BYTES"] = "4096"                          # the shipped library must not react
    n, k, l, D = 2, 256, 8, 3900
    p = params(n, k, l, M.bench_moduli(17))
    assert p._lib.pvw_build_is_tuning() == 0
    Pw = p.L * l
    item = (k + 1) * Pw * 8
    fills = sum_fills(D, None, chunk(item, D))
    assert len(fills) == 2 and fills[0] * item <= GIB < (fills[0] + 1) * item and D * item > GIB, fills
    rng = np.random.default_rng(1)
    c1s = rng.integers(0, 1 << 64, (D, k, p.L, l), dtype=np.uint64)
    c2s = rng.integers(0, 1 << 64, (D, n, p.L, l), dtype=np.uint64)
    w1, w2 = np.zeros((k, p.L, l), np.uint64), np.zeros((1, p.L, l), np.uint64)
    p._call("pvw_ct_sum_host", ptr(c1s), ptr(c2s), D, None, 0, 1, ptr(w1), ptr(w2), None)
    g1, g2, cnt = np.full_like(w1, MARK), np.full_like(w2, MARK), C.c_uint32()
    t0 = time.time()
    p._call("pvw_ct_sum", ptr(c1s), ptr(c2s), D, None, 0, 1, ptr(g1), ptr(g2), C.byref(cnt))
    dt = time.time() - t0
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and cnt.value == D
    print(f"real_bound: pieces {fills} of {item} bytes a dealer, pvw_ct_sum took {dt:.2f} s", flush=True)


CASES = {f.__name__[5:]: f for f in (case_sum, case_sum_decrypt, case_batch, case_all, case_encrypt, case_shamir, case_real_bound)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    _ffi.select("tuning")
    os.environ.pop("PVW_STAGE_BYTES", None)
    t0 = time.time()
    CASES[sys.argv[1]]()
    print(f"{sys.argv[1]}: {time.time() - t0:.1f} s")
    print("STAGED_PIECES_OK")

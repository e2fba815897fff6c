"""The concurrent-call promise (include/pvw_hip.h, Conventions) for the family over a prime field of up to 256
bits: pvw_shamir_shares_wide, pvw_deal_shares_wide[_rs], pvw_shamir_reconstruct_wide_checked / _corrected,
their _device forms and pvw_shamir_wide_from_limbs_device on streams of their own, and the two wide self-tests, from 8 threads
that share ONE context.  The machinery -- jobs with inputs of their own and sentinel-filled outputs, a barrier per round, the
serial run on a TWIN context, the overlap count, pvw_selftest_secret_residue afterwards -- is tests/_concurrent_worker.py's,
imported, as are its builders for the one-word calls that run beside the wide ones.  Every wide job is also held against its
*_host form and against Python's integers (`cpu`, which needs no GPU).  torch is imported FIRST so both libraries share one HIP
runtime.  Spawned case by case by tests/test_gpu_shamir_wide_concurrent.py; prints WIDE_CONCURRENT_OK (`selfcheck`: no GPU,
prints WIDE_CONCURRENT_SELFCHECK_OK)."""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _concurrent_worker import (GEOMS, STAGE_BYTES, THREADS, Dealt, Gen, Job, context, dev, dptr, expected, finish, full, host,  # noqa: E402
                                j_all, j_batch, j_ct_sum, j_deal, j_decode, j_encrypt, j_multi, j_reconstruct, j_sk, j_wire, mismatches,
                                overlapping_pairs, ptr, rotated_plans, run_threads, seed_block, sptr, text)
from _staged_pieces_worker import chunk, cut  # noqa: E402  (the library's piece arithmetic, restated)
from test_shamir_wide_host import BLS_R, COMPOSITE_255, SECP_N, W256, ints, restated_coeffs  # noqa: E402

P17, P64, P89, P255 = 65537, 2**64 + 13, 2**89 - 1, 2**255 - 19
PRIMES4 = (P17, P64, P255, SECP_N)
U64 = (1 << 64) - 1
CORRECT_PIECE_BYTES = 2048          # the `staged` case's PVW_CORRECT_PIECE_BYTES
CORRECT_PIECE_DEFAULT = 64 << 20    # correct_piece without it
POINTS = 140                        # party indices of the reconstructions are drawn below this
W = api._wide


def modw(pm):
    return api._wide_modulus(pm)


def big(g, pm):
    return int.from_bytes(g.rng.bytes(40), "little") % pm


def raised(v, pm, on):
    """v, or the largest word below 2^256 that means v mod p"""
    return v + pm * ((W256 - v) // pm) if on else v


def horner(coeffs, x, pm):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % pm
    return acc


def bare(geom):
    """a context of the geometry and nothing else: exists without a GPU (the *_host forms and the refusals need no more)"""
    n, k, l, moduli = GEOMS[geom]
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()


def wide_job(name, run, cpu, check=None, pieces=None):
    """cpu(ref) -> the expected tuple from the *_host form, held against Python's integers inside; no GPU"""
    def whole(ref, want):
        assert not mismatches([cpu(ref)], [want]), (name, "differs from the *_host form")
        if check:
            check(ref, want)
    j = Job(name, run, check=whole, pieces=pieces)
    j.cpu = cpu
    return j


# ---- the wide calls --------------------------------------------------------------------------------------------------------
def j_shares_wide(g, p0, D, t, pm, device=False):
    secrets = [raised(big(g, pm), pm, d % 2) for d in range(D)]
    seeds = [g.seed() for _ in range(D)]
    se, sd, pw = W(secrets), seed_block(seeds), modw(pm)

    def call(p, fn):
        out = full((D, p.n, 4))
        p._call(fn, ptr(se), D, t, ptr(pw), ptr(sd), None, ptr(out))
        return (out,)

    def run_device(p, s):
        with torch.cuda.stream(s):
            d_se, out = dev(se), dev(full((D, p.n, 4)))
            p._call("pvw_shamir_shares_wide_device", dptr(d_se), D, t, ptr(pw), ptr(sd), None, dptr(out), sptr(s))
            s.synchronize()
            return (host(out, np.uint64),)

    def cpu(ref):
        want = call(ref, "pvw_shamir_shares_wide_host")
        d = D - 1
        coeffs = [secrets[d] % pm] + restated_coeffs(seeds[d], t, pm)
        assert ints(want[0][d]) == [horner(coeffs, i + 1, pm) for i in range(ref.n)], ("Horner", D, t, pm)
        return want

    def check(ref, want):
        if device:
            assert not mismatches([call(ref, "pvw_shamir_shares_wide")], [want]), "the device form differs from the host-buffer form"
    return wide_job(f"shamir_shares_wide{'_device' if device else ''} D={D} t={t} {pm.bit_length()} bits",
                    run_device if device else lambda p, s: call(p, "pvw_shamir_shares_wide"), cpu, check,
                    pieces=lambda b, cb=0: cut(D, chunk((p0.n + 1) * 32, D, b)))


def deal_pieces(p0, D, NL, b):
    """deal_wide_host: whole dealers, half the budget, at least one"""
    per = (b // 2) // (NL * (p0.k + p0.n) * p0.L * p0.l * 8 + 32)
    return cut(D, min(max(per, 1), D))


def j_deal_wide(g, p0, D, pm, lb, repr, device=False):
    t = 2 + int(g.rng.integers(0, 4))
    NL = P.shamir_wide_limbs(pm, lb)
    V = D * NL
    secrets = [raised(big(g, pm), pm, d % 2) for d in range(D)]
    seeds = [g.seed() for _ in range(V)]
    se, sd, pw = W(secrets), seed_block(seeds), modw(pm)

    def call(p):
        c1, c2 = full((V, p.k, p.L, p.l)), full((V, p.n, p.L, p.l))
        p._call("pvw_deal_shares_wide", ptr(se), D, t, ptr(pw), lb, ptr(sd), ptr(c1), ptr(c2), repr)
        return c1, c2

    def run_device(p, s):
        with torch.cuda.stream(s):
            d_se, c1, c2 = dev(se), dev(full((V, p.k, p.L, p.l))), dev(full((V, p.n, p.L, p.l)))
            p._call("pvw_deal_shares_wide_device", dptr(d_se), D, t, ptr(pw), lb, ptr(sd), dptr(c1), dptr(c2), repr, sptr(s))
            s.synchronize()
            return host(c1, np.uint64), host(c2, np.uint64)

    def rows(ref):
        """the scalars of the V vectors: row d NL + w is limb w of dealer d's host shares, drawn under seeds[d NL]"""
        sh, out = full((D, ref.n, 4)), full((V, ref.n))
        ref._call("pvw_shamir_shares_wide_host", ptr(se), D, t, ptr(pw), ptr(seed_block(seeds[::NL])), None, ptr(sh))
        for d in range(D):
            api._check(ref._lib.pvw_shamir_wide_to_limbs_host(ptr(sh[d]), ref.n, lb, NL, ptr(out[d * NL:(d + 1) * NL])), ref._lib)
        d = D - 1
        coeffs = [secrets[d] % pm] + restated_coeffs(seeds[d * NL], t, pm)
        vals = [horner(coeffs, i + 1, pm) for i in range(ref.n)]
        assert out[d * NL:].tolist() == [[(v >> (w * lb)) & ((1 << lb) - 1) for v in vals] for w in range(NL)], ("limbs", D, pm)
        return out

    def check(ref, want):
        sc = rows(ref)
        c1, c2 = full((V, ref.k, ref.L, ref.l)), full((V, ref.n, ref.L, ref.l))
        ref._call("pvw_encrypt_multi", ptr(sc), V, ref.n, ptr(sd), ptr(c1), ptr(c2), repr)
        assert not mismatches([(c1, c2)], [want]), "the wide deal != encrypt_multi of the host shares' limb planes"
        if device:
            assert not mismatches([call(ref)], [want]), "the device form differs from the host-buffer form"
    j = Job(f"deal_shares_wide{'_device' if device else ''} D={D} V={V} repr={repr}", run_device if device else lambda p, s: call(p),
            check=check, pieces=lambda b, cb=0: deal_pieces(p0, D, NL, b))
    j.cpu = lambda ref: (rows(ref),)
    j.deal = (se, D, t, pw, lb, repr, V, NL)
    return j


def laid_out(rows, party_major):
    S, count = rows.shape[:2]
    return (np.ascontiguousarray(rows.transpose(1, 0, 2)), (1, S)) if party_major else (np.ascontiguousarray(rows), (count, 1))


def sharing(g, S, t, count, pm, points=POINTS):
    """S polynomials of degree t at `count` distinct points: (idx, polys, vals [S][count])"""
    polys = [[big(g, pm) for _ in range(t + 1)] for _ in range(S)]
    idx = g.rng.choice(points, count, replace=False).astype(np.uint64)
    return idx, polys, [[horner(a, int(i) + 1, pm) for i in idx] for a in polys]


def words(vals, pm):
    S, count = len(vals), len(vals[0])
    return W([raised(v, pm, (s + c) % 2) for s, row in enumerate(vals) for c, v in enumerate(row)]).reshape(S, count, 4)


def j_checked_wide(g, t, count, party_major, pm, S, device=False):
    idx, polys, vals = sharing(g, S, t, count, pm)
    bs, bc = int(g.rng.integers(0, S)), int(g.rng.integers(t + 1, count))
    vals[bs][bc] = (vals[bs][bc] + 1 + int(g.rng.integers(0, 1000))) % pm          # one deviating extra share
    arr, (ss, ps) = laid_out(words(vals, pm), party_major)
    pw = modw(pm)

    def call(p, fn, ctx=True):
        out, bad, col = full((S, 4)), full(S, np.uint32), full(count, np.uint32)
        args = (ptr(pw), t, ptr(idx), count, ptr(arr), S, ss, ps, ptr(out), ptr(bad), ptr(col))
        if ctx:
            p._call(fn, *args)
        else:
            api._check(getattr(p._lib, fn)(*args), p._lib)
        return out, bad, col

    def run_device(p, s):
        with torch.cuda.stream(s):
            d_sh, out, bad, col = dev(arr), dev(full((S, 4))), dev(full(S, np.uint32)), dev(full(count, np.uint32))
            p._call("pvw_shamir_reconstruct_wide_checked_device", ptr(pw), t, ptr(idx), count, dptr(d_sh), S, ss, ps, dptr(out), dptr(bad),
                    dptr(col), sptr(s))
            s.synchronize()
            return host(out, np.uint64), host(bad, np.uint32), host(col, np.uint32)

    def cpu(ref):
        want = call(ref, "pvw_shamir_reconstruct_wide_checked_host", False)
        assert ints(want[0]) == [a[0] for a in polys], "the secrets"
        assert want[1].tolist() == [int(s == bs) for s in range(S)] and want[2].tolist() == [int(c == bc) for c in range(count)]
        return want

    def check(ref, want):
        if device:
            assert not mismatches([call(ref, "pvw_shamir_reconstruct_wide_checked")], [want]), "the device form differs from the host-buffer form"
    name = f"reconstruct_wide_checked{'_device' if device else ''} ({t}, {count}) S={S} {'party' if party_major else 'secret'}-major"
    return wide_job(name, run_device if device else lambda p, s: call(p, "pvw_shamir_reconstruct_wide_checked"), cpu, check,
                    pieces=lambda b, cb=0: cut(S, chunk((count + 1) * 32 + 4, S, b)))


def corrected_pieces(t, count, S, b, cb):
    """pvw_shamir_reconstruct_wide_corrected: the staging piece, no larger than one pass over the kernels (correct_piece)"""
    r = count - t - 1
    per = chunk((count + 1) * 32 + (count + 63) // 64 * 8 + 4, S, b)
    cap = min(max(cb // ((count + r + r // 2 + 1) * 32 + 4), 1), 65535 * 4, S)
    return cut(S, min(per, cap))


def j_corrected_wide(g, t, count, party_major, pm, S, device=False, points=POINTS, host_form=True):
    """host_form False: the planted truth alone (Berlekamp-Welch on the host is cubic in count)"""
    r = count - t - 1
    E, nw = r // 2, (count + 63) // 64
    idx, polys, vals = sharing(g, S, t, count, pm, points)
    plan = []
    for s in range(S):                                              # E, 1, 0, E / 2 wrong columns in turn, never more than E
        cols = g.rng.choice(count, (E, 1, 0, E // 2)[s % 4], replace=False).tolist()
        if s == 0 and 0 not in cols:
            cols[0] = 0                                             # column 0: the checked call's first basis column
        plan.append(sorted(cols))
        for c in cols:
            vals[s][c] = (vals[s][c] + 1 + big(g, pm - 1)) % pm
    assert E >= 1 and all(len(cols) <= E for cols in plan) and 0 in plan[0], plan
    arr, (ss, ps) = laid_out(words(vals, pm), party_major)
    pw = modw(pm)
    truth = (W([a[0] for a in polys]), np.array([len(cols) for cols in plan], np.uint32),
             np.bincount([c for cols in plan for c in cols], minlength=count).astype(np.uint32),
             np.array([[sum(1 << (c % 64) for c in cols if c // 64 == w) for w in range(nw)] for cols in plan], np.uint64))

    def call(p, fn, ctx=True):
        out, nerr, col, mask = full((S, 4)), full(S, np.uint32), full(count, np.uint32), full((S, nw))
        args = (ptr(pw), t, ptr(idx), count, ptr(arr), S, ss, ps, ptr(out), ptr(nerr), ptr(col), ptr(mask))
        if ctx:
            p._call(fn, *args)
        else:
            api._check(getattr(p._lib, fn)(*args), p._lib)
        return out, nerr, col, mask

    def run_device(p, s):
        with torch.cuda.stream(s):
            d_sh, out, nerr, col, mask = dev(arr), dev(full((S, 4))), dev(full(S, np.uint32)), dev(full(count, np.uint32)), dev(full((S, nw)))
            p._call("pvw_shamir_reconstruct_wide_corrected_device", ptr(pw), t, ptr(idx), count, dptr(d_sh), S, ss, ps, dptr(out), dptr(nerr),
                    dptr(col), dptr(mask), sptr(s))
            s.synchronize()
            return host(out, np.uint64), host(nerr, np.uint32), host(col, np.uint32), host(mask, np.uint64)

    def cpu(ref):
        if not host_form:
            return truth
        want = call(ref, "pvw_shamir_reconstruct_wide_corrected_host", False)     # Berlekamp-Welch
        assert not mismatches([want], [truth]), "the host form differs from the planted secrets, nerr, col_err or err_mask"
        return want

    def check(ref, want):
        if device:
            assert not mismatches([call(ref, "pvw_shamir_reconstruct_wide_corrected")], [want]), "the device form differs from the host-buffer form"
    name = f"reconstruct_wide_corrected{'_device' if device else ''} ({t}, {count}) E={E} S={S} {'party' if party_major else 'secret'}-major"
    j = wide_job(name, run_device if device else lambda p, s: call(p, "pvw_shamir_reconstruct_wide_corrected"), cpu, check,
                 pieces=lambda b, cb=CORRECT_PIECE_DEFAULT: corrected_pieces(t, count, S, b, cb))
    j.plan, j.E = plan, E
    return j


def j_fold_device(g, NL, lb, pm, count=70):
    """both stride pairs on the calling thread's stream: the planes [NL][count] and the limbs of an element side by side"""
    planes = g.rng.integers(0, 1 << 64, size=(NL, count), dtype=np.uint64)
    planes[0, 0], planes[NL - 1, count - 1] = np.uint64(U64), np.uint64(U64)
    side = np.ascontiguousarray(planes.T)
    pw = modw(pm)

    def run(p, s):
        with torch.cuda.stream(s):
            d_pl, d_sd, o1, o2 = dev(planes), dev(side), dev(full((count, 4))), dev(full((count, 4)))
            p._call("pvw_shamir_wide_from_limbs_device", ptr(pw), dptr(d_pl), count, count, 1, lb, NL, dptr(o1), sptr(s))
            p._call("pvw_shamir_wide_from_limbs_device", ptr(pw), dptr(d_sd), count, 1, NL, lb, NL, dptr(o2), sptr(s))
            s.synchronize()
            return host(o1, np.uint64), host(o2, np.uint64)

    def cpu(ref):
        out = full((count, 4))
        api._check(ref._lib.pvw_shamir_wide_from_limbs_host(ptr(pw), ptr(planes), count, lb, NL, ptr(out)), ref._lib)
        assert ints(out) == [sum(int(planes[w, i]) << (w * lb) for w in range(NL)) % pm for i in range(count)], ("fold", NL, lb)
        return out, out
    return wide_job(f"wide_from_limbs_device NL={NL} limb_bits={lb}", run, cpu)


def j_selftest_wide(g, pm):
    """pvw_selftest_shamir_wide_step and _mul on 40 operands each, 0, 1 and p - 1 among them"""
    cnt = 40
    edge = [0, 1, pm - 1]
    acc, add, a, b = ([edge[(i + o) % 3] if i < 9 else big(g, pm) for i in range(cnt)] for o in (0, 1, 0, 2))
    b[:9] = [edge[i // 3] for i in range(9)]                          # with a: every pair of edge operands
    x = np.array([(1, (1 << 32) - 1, 2)[i % 3] if i < 9 else int(g.rng.integers(0, 1 << 32)) for i in range(cnt)], np.uint64)
    wa, wd, ma, mb, pw = W(acc), W(add), W(a), W(b), modw(pm)

    def run(p, s):
        o1, o2 = full((cnt, 4)), full((cnt, 4))
        p._call("pvw_selftest_shamir_wide_step", ptr(pw), ptr(wa), ptr(x), ptr(wd), cnt, ptr(o1))
        p._call("pvw_selftest_shamir_wide_mul", ptr(pw), ptr(ma), ptr(mb), cnt, ptr(o2))
        return o1, o2

    def cpu(ref):
        return (W([(u * int(v) + w) % pm for u, v, w in zip(acc, x, add)]), W([u * v % pm for u, v in zip(a, b)]))
    return wide_job(f"selftest wide step + mul {pm.bit_length()} bits", run, cpu)


def j_chain(g, p0, sk):
    """nothing leaves the device between the steps: deal (five dealers, t = 1, the secp256k1 order) -> the first five parties
    decrypt every limb of every dealer (pvw_decrypt_all_device, [party][dealer NL + w]) -> the fold in place, strides (1, NL),
    to [party][dealer][4] -> checked reconstruction in place, strides (1, D), every dealer a secret: the dealt secrets, nothing
    flagged (the shape of the `loop` case of tests/_shamir_wide_checked_worker.py)"""
    NP, D, t, pm, lb = 5, 5, 1, SECP_N, 52
    NL = P.shamir_wide_limbs(pm, lb)
    V = D * NL
    secrets = [pm - 1 - big(g, 1 << 100) for _ in range(D)]
    seeds = [g.seed() for _ in range(V)]
    se, sd, pw, idx = W(secrets), seed_block(seeds), modw(pm), np.arange(NP, dtype=np.uint64)

    def run(p, s):
        N = P.REPR_NTT
        with torch.cuda.stream(s):
            d_se, c1, c2, d_sk = dev(se), dev(full((V, p.k, p.L, p.l))), dev(full((V, p.n, p.L, p.l))), dev(sk[:NP])
            limbs, folded = dev(full((NP, V))), dev(full((NP * D, 4)))
            out, bad, col = dev(full((D, 4))), dev(full(D, np.uint32)), dev(full(NP, np.uint32))
            p._call("pvw_deal_shares_wide_device", dptr(d_se), D, t, ptr(pw), lb, ptr(sd), dptr(c1), dptr(c2), N, sptr(s))
            p._call("pvw_decrypt_all_device", 0, NP, dptr(d_sk), dptr(c1), dptr(c2), V, N, dptr(limbs), sptr(s))
            p._call("pvw_shamir_wide_from_limbs_device", ptr(pw), dptr(limbs), NP * D, 1, NL, lb, NL, dptr(folded), sptr(s))
            p._call("pvw_shamir_reconstruct_wide_checked_device", ptr(pw), t, ptr(idx), NP, dptr(folded), D, 1, D, dptr(out), dptr(bad),
                    dptr(col), sptr(s))
            s.synchronize()
            return host(out, np.uint64), host(bad, np.uint32), host(col, np.uint32), host(folded, np.uint64)

    def cpu(ref):
        sh = full((D, ref.n, 4))
        ref._call("pvw_shamir_shares_wide_host", ptr(se), D, t, ptr(pw), ptr(seed_block(seeds[::NL])), None, ptr(sh))
        coeffs = [secrets[0]] + restated_coeffs(seeds[0], t, pm)
        assert ints(sh[0]) == [horner(coeffs, i + 1, pm) for i in range(ref.n)]
        return (W(secrets), np.zeros(D, np.uint32), np.zeros(NP, np.uint32), np.ascontiguousarray(sh[:, :NP].transpose(1, 0, 2)).reshape(NP * D, 4))
    return wide_job("deal_wide -> decrypt_all -> fold -> reconstruct_wide_checked, on the device", run, cpu)


# ---- the job lists ---------------------------------------------------------------------------------------------------------
def prime(i):
    return PRIMES4[i % 4]


def cold_round(p0, r):
    """the eight first calls of a context: all of them wide, apart from one pvw_encrypt"""
    g = Gen(11, r)
    N = P.REPR_NTT
    return [j_deal_wide(g, p0, 1, P89, 52, N), j_corrected_wide(g, 3, 12, r % 2 == 1, prime(r), 4), j_checked_wide(g, 3, 9, r % 2 == 0, prime(r + 1), 5),
            j_shares_wide(g, p0, 3 if r % 2 else 7, 2 + r, prime(r + 2)), j_deal_wide(g, p0, 2, SECP_N, 52, P.REPR_POWER if r == 1 else N),
            j_corrected_wide(g, 5, 136, r % 2 == 0, prime(r + 3), 2), j_checked_wide(g, 33, 70, r % 2 == 1, prime(r + 2), 3), j_encrypt(g, p0)]


def bare_round(p0, r):
    """eight wide calls that need no matrices: the correction at count 2052, t 1, E 1025 among them, whose Berlekamp-Massey launch
    asks for 2 * 1026 * 32 = 65 664 bytes of LDS, more than a launch gets unless init_shamir_attributes has raised the limit
    (planted truth: the cubic host form cannot run at this size); three device forms on streams the context has never seen,
    whose workspaces enter the stream map while the other threads run"""
    g = Gen(12, r)
    return [j_corrected_wide(g, 1, 2052, False, SECP_N, 2, points=1 << 20, host_form=False), j_checked_wide(g, 33, 70, r % 2 == 0, prime(r), 3),
            j_shares_wide(g, p0, 7, 9 - r, prime(r + 1), True), j_corrected_wide(g, 5, 136, r % 2 == 1, prime(r + 2), 2), j_selftest_wide(g, prime(r + 3)),
            j_checked_wide(g, 3, 9, r % 2 == 1, prime(r + 1), 5, True), j_fold_device(g, 5, 52, SECP_N),
            j_corrected_wide(g, 3, 12, r % 2 == 0, prime(r), 4, True)]


def mixed_wide(p0, r, tag):
    """sixteen wide jobs: every host-buffer call, the fold on the thread's stream and the self-tests; the shapes on either side of
    each dispatch, the V = 135 deal (two passes of the share scratch) and the E = 65 correction (two blocks of the locator)"""
    g = Gen(tag, r, p0.n)
    N, PW = P.REPR_NTT, P.REPR_POWER
    pm = lambda i: prime(i + r)
    return [
        j_deal_wide(g, p0, 27, SECP_N, 52, N), j_checked_wide(g, 3, 9, False, pm(0), 4), j_shares_wide(g, p0, 3, 2 + (r + 5) % 8, pm(1)),
        j_corrected_wide(g, 3, 12, True, pm(2), 5), j_deal_wide(g, p0, 1, P89, 52, PW), j_fold_device(g, 5, 52, SECP_N),
        j_checked_wide(g, 33, 70, True, pm(3), 3), j_corrected_wide(g, 5, 136, False, pm(0), 2),
        j_shares_wide(g, p0, 7, 2 + (r + 2) % 8, pm(2)), j_deal_wide(g, p0, 2, SECP_N, 52, PW), j_selftest_wide(g, pm(1)),
        j_checked_wide(g, 3, 9, True, pm(3), 6), j_corrected_wide(g, 3, 12, False, pm(1), 4), j_deal_wide(g, p0, 1, P89, 52, N),
        j_fold_device(g, 16, 16, BLS_R), j_checked_wide(g, 33, 70, False, pm(2), 4),
    ]


def mixed_round(p0, dt, r, tag):
    """32 jobs, thread t takes every 8th: a wide call, a one-word call or an encrypt, a wide call, ... (dt None: the wide half)"""
    wide = mixed_wide(p0, r, tag)
    if dt is None:
        return wide
    g = Gen(tag + 1, r, p0.n)
    N, PW = P.REPR_NTT, P.REPR_POWER
    rest = [
        j_encrypt(g, p0), j_multi(g, p0, 5), j_batch(g, p0, dt, "plain", N), j_all(g, p0, dt, "checked", 5, N), j_ct_sum(g, p0, dt, True),
        j_deal(g, p0, 6), j_reconstruct(g, p0, 3, 9, False), j_wire(g, p0),
        j_decode(g, p0, "plain"), j_sk(g, p0, dt), j_encrypt(g, p0, PW), j_multi(g, p0, 2, PW), j_all(g, p0, dt, "values", 40, N),
        j_deal(g, p0, 2, PW), j_reconstruct(g, p0, 5, 12, True), j_batch(g, p0, dt, "plain", PW),
    ]
    return wide[:8] + rest[:8] + wide[8:] + rest[8:]


def staged_round(p0, r):
    """every wide host-buffer call that stages, sized for three pieces or more at STAGE_BYTES / CORRECT_PIECE_BYTES"""
    g = Gen(13, r, p0.n)
    N, PW = P.REPR_NTT, P.REPR_POWER
    pm = lambda i: prime(i + r)
    return [
        j_shares_wide(g, p0, 3, 4, pm(0)), j_deal_wide(g, p0, 3, SECP_N, 52, N), j_checked_wide(g, 3, 9, False, pm(1), 14),
        j_corrected_wide(g, 3, 12, False, pm(2), 7), j_checked_wide(g, 33, 70, True, pm(3), 4), j_corrected_wide(g, 5, 136, True, pm(0), 3),
        j_deal_wide(g, p0, 4, P89, 52, PW), j_shares_wide(g, p0, 7, 9, pm(1)),
        j_corrected_wide(g, 3, 12, True, pm(3), 6), j_checked_wide(g, 33, 70, False, pm(0), 3), j_deal_wide(g, p0, 3, SECP_N, 52, PW),
        j_shares_wide(g, p0, 5, 2, pm(2)), j_checked_wide(g, 3, 9, True, pm(2), 13), j_deal_wide(g, p0, 3, P89, 52, N),
        j_corrected_wide(g, 5, 136, False, pm(1), 3), j_shares_wide(g, p0, 4, 7, pm(3)),
    ]


def staged_pieces(rounds, say=False):
    """up front, from the piece arithmetic: one piece at the library's budgets, three or more at the case's"""
    for jobs in rounds:
        for j in jobs:
            one, many = j.pieces(1 << 30), j.pieces(STAGE_BYTES, CORRECT_PIECE_BYTES)
            assert len(one) == 1 and len(many) >= 3, (j.name, one, many)
            if say:
                print(f"staged {j.name}: pieces {many if len(many) < 12 else str(len(many)) + ' in all'}", flush=True)


def streams_round(p0, sk, r):
    """(jobs, plan): threads 0..3 issue the device forms and the chain on streams of their own, threads 4 and 5 make wide
    host-buffer calls"""
    g = Gen(15, r)
    N = P.REPR_NTT
    jobs, plan = [], []
    for t in range(4):
        kinds = [lambda: j_shares_wide(g, p0, 7, 2 + (t + r) % 8, prime(t + r), True), lambda: j_deal_wide(g, p0, 2 if t % 2 else 1, SECP_N if t % 2 else P89, 52, N, True),
                 lambda: j_checked_wide(g, *((33, 70) if (t + r) % 2 else (3, 9)), t % 2 == 0, prime(t), 4, True),
                 lambda: j_corrected_wide(g, *((5, 136) if (t + r) % 2 else (3, 12)), t % 2 == 1, prime(t + 1), 2 if (t + r) % 2 else 4, True),
                 lambda: j_chain(g, p0, sk), lambda: j_fold_device(g, *((5, 52, SECP_N) if t % 2 else (16, 16, BLS_R)))]
        mine = [kinds[(t + r + x) % 6]() for x in range(4)]
        plan.append(list(range(len(jobs), len(jobs) + len(mine))))
        jobs += mine
    for t in range(2):
        mine = [j_deal_wide(g, p0, 2, SECP_N, 52, N), j_checked_wide(g, 3, 9, False, prime(r), 5), j_corrected_wide(g, 5, 136, True, prime(r + 1), 2),
                j_shares_wide(g, p0, 3, 3 + r, prime(r + 2))] if t == 0 else \
               [j_corrected_wide(g, 3, 12, False, prime(r + 3), 4), j_deal_wide(g, p0, 1, P89, 52, P.REPR_POWER), j_shares_wide(g, p0, 7, 9 - r, prime(r)),
                j_checked_wide(g, 33, 70, True, prime(r + 2), 3)]
        plan.append(list(range(len(jobs), len(jobs) + len(mine))))
        jobs += mine
    return jobs, plan


RS_SHAPES = [(1, P89, 52), (2, SECP_N, 52), (3, P17, 16), (1, SECP_N, 52)]     # D NL = 2 (VALU), 10, 6, 5 (matrix cores)


def errors_round(p0, r):
    """the fourteen valid wide jobs of the seven other threads"""
    g = Gen(17, r)
    N = P.REPR_NTT
    jobs = []
    for t in range(THREADS - 1):
        jobs += [(j_shares_wide(g, p0, 3, 2 + t, prime(t)), j_checked_wide(g, 3, 9, t % 2 == 0, prime(t + 1), 4),
                  j_deal_wide(g, p0, 1, P89, 52, N), j_selftest_wide(g, prime(t)))[(t + r) % 4],
                 (j_corrected_wide(g, 3, 12, t % 2 == 1, prime(t + 2), 4), j_deal_wide(g, p0, 2, SECP_N, 52, N),
                  j_checked_wide(g, 33, 70, t % 2 == 1, prime(t + 3), 3))[(t + r) % 3]]
    return jobs


# ---- refused calls ---------------------------------------------------------------------------------------------------------
def refused_expect(n):
    return [(1, "plain_modulus must be prime (Shamir shares live in a field)"),
            (1, "plain_modulus must be an odd prime (Shamir shares live in a field)"),
            (1, f"degree {n} needs more than {n} parties"), (1, "limb_bits must be in [16, 62]"), (1, "duplicate party index"),
            (1, "NULL argument")]


def refused_calls(p, accept_fn, times):
    """`times` over: each refused wide call behind an accepted one with the secp256k1 order on the same thread (the thread's
    cached verdict on the last prime must not let the composite through, nor the cache forget the prime); returns the codes
    and the messages; the outputs keep their sentinel"""
    n, lib = p.n, p._lib
    secp, comp, even = modw(SECP_N), modw(COMPOSITE_255), modw(SECP_N - 1)
    se, sd, good = W([5]), np.zeros(32, np.uint8), full((1, n, 4))
    sh = full((1, n, 4))
    idx, dup = np.arange(4, dtype=np.uint64), np.array([0, 1, 2, 1], np.uint64)
    rows, out, cnt, col, mask = W(list(range(8))), full((2, 4)), full(2, np.uint32), full(4, np.uint32), full((2, 1))
    calls = (lambda: lib.pvw_shamir_shares_wide(p._h, ptr(se), 1, 1, ptr(comp), ptr(sd), None, ptr(sh)),                    # a composite of 255 bits
             lambda: lib.pvw_shamir_reconstruct_wide_checked(p._h, ptr(even), 1, ptr(idx), 4, ptr(rows), 2, 4, 1, ptr(out), ptr(cnt), ptr(col)),   # even
             lambda: lib.pvw_shamir_shares_wide(p._h, ptr(se), 1, n, ptr(secp), ptr(sd), None, ptr(sh)),                     # degree >= n
             lambda: lib.pvw_shamir_wide_from_limbs_device(p._h, ptr(secp), None, 0, 1, 1, 15, 5, None, None),               # limb_bits 15
             lambda: lib.pvw_shamir_reconstruct_wide_corrected(p._h, ptr(secp), 1, ptr(dup), 4, ptr(rows), 2, 4, 1, ptr(out), ptr(cnt), ptr(col),
                                                               ptr(mask)),                                                   # a duplicate index
             lambda: lib.pvw_shamir_reconstruct_wide_checked(p._h, ptr(secp), 1, ptr(idx), 4, ptr(rows), 2, 4, 1, None, ptr(cnt), ptr(col)))   # NULL output
    seen = []
    for _ in range(times):
        for call in calls:
            api._check(getattr(lib, accept_fn)(p._h, ptr(se), 1, 1, ptr(secp), ptr(sd), None, ptr(good)), lib)
            rc = call()
            seen.append((rc, _ffi.last_error(lib)))
    for a in (sh, out, cnt, col, mask):
        assert (a == full(a.shape, a.dtype)).all(), "a refused call wrote to its outputs"
    assert ints(good[0]) == [horner([5] + restated_coeffs(bytes(32), 1, SECP_N), i + 1, SECP_N) for i in range(n)], "the accepted call"
    return seen


def packed_seen(seen):
    return np.array([rc for rc, _ in seen], np.int32), text("|".join(m for _, m in seen))


def watched(job):
    """the job, and the calling thread's pvw_last_error behind it: a thread whose calls all succeed never sees another's text"""
    def run(p, s):
        return job.run(p, s) + (text(_ffi.last_error(p._lib)),)

    def check(ref, want):
        assert want[-1].size == 0, ("a succeeding thread has an error message", bytes(want[-1]))
        job.check(ref, want[:-1])
    return Job(job.name, run, check=check)


# ---- the CPU-only checks ---------------------------------------------------------------------------------------------------
def in_thread(fn):
    """fn() on a thread of its own, so that its refusals do not become the main thread's pvw_last_error"""
    box = []
    th = threading.Thread(target=lambda: box.append(fn()))
    th.start()
    th.join()
    assert box, "the helper thread failed"
    return box[0]


def selfcheck(whole=True):
    g = Gen(0)
    ref = bare("plain")
    # the comparison can fail: real expected values of three jobs, then swapped, one bit flipped, one missing
    want = [j.cpu(ref) for j in (j_checked_wide(g, 3, 9, False, SECP_N, 4), j_checked_wide(g, 3, 9, False, SECP_N, 4),
                                 j_corrected_wide(g, 3, 12, True, P64, 4), j_shares_wide(g, ref, 3, 2, P255))]
    same = [tuple(a.copy() for a in w) for w in want]
    assert mismatches(same, want) == []
    swapped = list(same)
    swapped[0], swapped[1] = swapped[1], swapped[0]                   # a result handed to the wrong call of the same kind
    assert mismatches(swapped, want) == [0, 1]
    flipped = [tuple(a.copy() for a in w) for w in want]
    flipped[3][0][2, 5, 3] ^= np.uint64(1 << 63)                     # one bit of one share
    assert mismatches(flipped, want) == [3]
    assert mismatches(same[:3] + [None], want) == [3] and mismatches(same[:2], want) == [2, 3]
    assert overlapping_pairs([(0, 0.0, 1.0), (1, 0.5, 1.5), (1, 2.0, 3.0), (0, 2.5, 2.6)]) == 2
    assert overlapping_pairs([(0, 0.0, 1.0), (0, 0.5, 1.5), (1, 1.5, 2.0)]) == 0
    # the refused calls, serially: they refuse before any device work
    for geom in ("plain", "packed56"):
        p = bare(geom)
        seen = in_thread(lambda: refused_calls(p, "pvw_shamir_shares_wide_host", 2))
        assert seen == refused_expect(p.n) * 2, seen
    if whole:
        # every case's wide jobs: the *_host forms against Python's integers, the planted rows within E
        lists = [cold_round(bare("packed56"), 0), mixed_round(bare("plain"), None, 0, 21), staged_round(ref, 0),
                 streams_round(bare("packed56"), None, 0)[0], errors_round(bare("packed56"), 0), bare_round(ref, 0)]
        staged_pieces([staged_round(ref, r) for r in range(3)])
        done = 0
        for jobs, geom in zip(lists, ("packed56", "plain", "plain", "packed56", "packed56", "plain")):
            p = bare(geom)
            for j in jobs:
                if hasattr(j, "plan"):
                    assert all(len(cols) <= j.E for cols in j.plan) and max(len(cols) for cols in j.plan) == j.E, (j.name, j.plan)
                if hasattr(j, "cpu"):
                    j.cpu(p)
                    done += 1
        print(f"selfcheck: {done} wide jobs held against Python's integers", flush=True)
    print("cases:", " ".join(sorted(CASES)))
    print("WIDE_CONCURRENT_SELFCHECK_OK")


# ---- the cases -------------------------------------------------------------------------------------------------------------
def cold():
    """8 threads make a fresh context's FIRST calls together, all of them wide apart from one pvw_encrypt: two deals (V = 2 on
    the VALU, V = 10 on the matrix cores: the share scratch, ensure_xm and the GEMM buffers built concurrently), two corrected
    and two checked reconstructions, the shares alone.  No pvw_prepare, no warm-up."""
    geom = "packed56"
    ref, ref_gpk, _ = context(geom, False)
    rounds = [cold_round(ref, r) for r in range(3)]
    want = expected(ref, rounds, True)
    p, gpk, _ = context(geom, False)                                # the shared context: nothing but the loads has run on it
    got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS, 0), THREADS)
    finish(f"cold {geom}", p, rounds, want, got, spans, errors, True)


def cold_bare():
    """8 threads make the first calls of a context that has loaded NOTHING: no CRS, no key, so the device has not been touched
    for it and ensure_device itself (the tables, the kernel attributes, init_shamir_attributes among them) is entered by eight
    wide calls at once -- one of them a correction whose launch needs the LDS limit that ensure_device raises.  The twin runs
    AFTER the threads: its own initialisation must not be what set the attribute."""
    p = bare("plain")
    rounds = [bare_round(p, r) for r in range(2)]
    got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS, 0), THREADS)
    want = expected(bare("plain"), rounds, True)
    finish("cold-bare", p, rounds, want, got, spans, errors, True)


def mixed(geom):
    """keys from pvw_keygen, then 32 jobs per round on 8 threads, wide and one-word kinds in turn, the list rotated by 5 from
    round to round: a recycled workspace goes from a wide call to a one-word call or an encrypt, and back"""
    ref, ref_gpk, ref_parties = context(geom, True)
    dt = Dealt(ref, ref_gpk, ref_parties)
    rounds = [mixed_round(ref, dt, r, 21) for r in range(3)]
    want = expected(ref, rounds, ref.sum_capacity() >= dt.D)
    p, gpk, parties = context(geom, True)
    got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS), THREADS)
    finish(f"mixed {geom}", p, rounds, want, got, spans, errors, True)


def staged():
    """the tuning build with PVW_STAGE_BYTES = 2048 and PVW_CORRECT_PIECE_BYTES = 2048: every wide host-buffer call takes three
    pieces or more, so a workspace is held across several copies while the other threads run; expected values: one piece each,
    on the twin"""
    if not os.path.exists(_ffi.LIB_TUNING_PATH):
        print("WIDE_CONCURRENT_SKIP the tuning build is absent")
        return False
    _ffi.select("tuning")
    names = {"PVW_STAGE_BYTES": STAGE_BYTES, "PVW_CORRECT_PIECE_BYTES": CORRECT_PIECE_BYTES}
    for name in names:
        os.environ.pop(name, None)
    ref, ref_gpk, _ = context("plain", False)
    assert ref._lib.pvw_build_is_tuning() == 1
    rounds = [staged_round(ref, r) for r in range(3)]
    staged_pieces(rounds[:1], say=True)
    staged_pieces(rounds[1:])
    want = expected(ref, rounds, True)                               # one piece each
    p, gpk, _ = context("plain", False)
    for name, value in names.items():
        os.environ[name] = str(value)
    try:
        got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS), THREADS)
    finally:
        for name in names:
            os.environ.pop(name, None)
    finish("staged plain", p, rounds, want, got, spans, errors, True)
    return True


def streams():
    """after pvw_prepare(PVW_PREPARE_MFMA) and one sizing call for each stream, 4 threads issue the wide device forms and the
    chain on a stream of their own (the async_ws map under mu, correct_wide and the share scratch of each stream's workspace)
    while 2 threads make wide host-buffer calls (the pool)"""
    geom, T = "packed56", 6
    ref, ref_gpk, ref_parties = context(geom, True)
    sk = Dealt(ref, ref_gpk, ref_parties).sk
    made = [streams_round(ref, sk, r) for r in range(3)]
    rounds, plans = [m[0] for m in made], [m[1] for m in made]
    want = expected(ref, rounds, True)
    p, gpk, parties = context(geom, True)
    ss = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(T)]
    for i, s in enumerate(ss[:4]):
        p.prepare(_ffi.PREPARE_MFMA, s.cuda_stream)
        # the largest corrected layout of the case: the threads' calls find correct_wide sized
        sizing = j_corrected_wide(Gen(16, i), 5, 136, False, SECP_N, 2, True)
        assert not mismatches([sizing.run(p, s)], [sizing.cpu(ref)]), "the sizing call"
    got, spans, errors = run_threads(p, rounds, plans, T, ss)
    finish(f"streams {geom}", p, rounds, want, got, spans, errors, True)


def rs():
    """every thread deals from a pvw_rnd_state of its own: 3 calls of pvw_deal_shares_wide_rs, in turn with its _device form on the
    thread's stream, each equal to the seeded deal under call_seed(S, c + v); each counter ends at c plus the sum of D NL"""
    geom = "packed56"
    ref, ref_gpk, _ = context(geom, False)
    p, gpk, _ = context(geom, False)
    g = Gen(18)
    states, starts = [], []
    for t in range(THREADS):
        S, c = g.seed(), int(g.rng.integers(0, 1 << 40))
        states.append((S, P.DeviceRandomness(p, S, c)))
        starts.append(c)
    rounds, want, cur = [], [], list(starts)
    for r in range(3):
        jobs, row = [], []
        for t in range(THREADS):
            D, pm, lb = RS_SHAPES[(t + r) % 4]
            S, st = states[t]
            repr = P.REPR_POWER if (t + r) % 3 == 0 else P.REPR_NTT
            seeded = j_deal_wide(g, ref, D, pm, lb, repr)
            se, D, deg, pw, lb, repr, V, NL = seeded.deal
            sd = seed_block([P.DeviceRandomness.call_seed(S, cur[t] + v) for v in range(V)])
            cur[t] += V
            c1, c2 = full((V, ref.k, ref.L, ref.l)), full((V, ref.n, ref.L, ref.l))
            ref._call("pvw_deal_shares_wide", ptr(se), D, deg, ptr(pw), lb, ptr(sd), ptr(c1), ptr(c2), repr)

            def run(q, s, a=(se, D, deg, pw, lb, repr, V), st=st, device=(t + r) % 2 == 1):
                se, D, deg, pw, lb, repr, V = a
                o1, o2 = full((V, q.k, q.L, q.l)), full((V, q.n, q.L, q.l))
                if not device:
                    q._call("pvw_deal_shares_wide_rs", ptr(se), D, deg, ptr(pw), lb, st._h, ptr(o1), ptr(o2), repr)
                    return o1, o2
                with torch.cuda.stream(s):                           # the _device form on the thread's stream, drained before it returns
                    d_se, d1, d2 = dev(se), dev(o1), dev(o2)
                    q._call("pvw_deal_shares_wide_rs_device", dptr(d_se), D, deg, ptr(pw), lb, st._h, dptr(d1), dptr(d2), repr, sptr(s))
                    s.synchronize()
                    return host(d1, np.uint64), host(d2, np.uint64)
            jobs.append(Job(f"deal_shares_wide_rs{'_device' if (t + r) % 2 else ''} D={D} V={V}", run, want=(c1, c2)))
            row.append((c1, c2))
        rounds.append(jobs)
        want.append(row)
    got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS, 0), THREADS)
    finish(f"rs {geom}", p, rounds, want, got, spans, errors, True)
    ends = [st.counter() for _, st in states]
    assert ends == cur, ("counters", ends, cur)
    for _, st in states:
        st.free()
    print(f"rs: counters advanced by {[e - s for e, s in zip(ends, starts)]}", flush=True)


def errors():
    """one thread makes refused wide calls, 40 times each of six, every one behind an accepted call with the secp256k1 order
    (wide_modulus_check's per-thread verdict), while seven threads run valid wide jobs: the refused calls get their code and
    message every time and write nothing, the valid results are exact, and no succeeding thread's pvw_last_error shows
    another's text"""
    geom = "packed56"
    ref, ref_gpk, _ = context(geom, False)
    want_refused = packed_seen(refused_expect(ref.n) * 40)
    rounds = [[Job("refused wide calls", lambda p, s: packed_seen(refused_calls(p, "pvw_shamir_shares_wide", 40)), want=want_refused)]
              + [watched(j) for j in errors_round(ref, r)] for r in range(3)]
    want = expected(ref, rounds, True)
    p, gpk, _ = context(geom, False)
    plans = [[[0]] + [[2 * t - 1, 2 * t] for t in range(1, THREADS)] for _ in rounds]     # thread 0: the refused calls
    got, spans, errs = run_threads(p, rounds, plans, THREADS)
    finish(f"errors {geom}", p, rounds, want, got, spans, errs, True)


def default_stream():
    """A stream's FIRST deals are enqueued while the legacy default stream is busy (a sleep kernel stands for what a framework
    queues there).  hipMemset returns to the host before the fill has run, and the default stream it runs on is not ordered
    against the library's non-blocking streams: a fresh block that is zeroed that way and then written by the stream's kernels
    (the share scratch, r-hat) loses what they wrote when the fill lands later.  Six deals, wide (500 limb vectors) and
    one-word (512 dealers) in turn, go back to back on a stream the context has never seen, 16 times over on as many streams,
    behind sleeps spread from 0.2 ms to past the end of the deals as timed on the twin, so that some end while shares are in
    flight; every deal equals the twin's, made with the default stream idle.  (With the fills not waited for, 5 of the 16
    attempts gave a wrong deal, the later the sleep ended the later the deal.)  The timing can only let a wrong library pass,
    never fail a right one."""
    geom = "packed56"
    ref, ref_gpk, _ = context(geom, False)
    g = Gen(19)
    N, PM, t, pw = P.REPR_NTT, (1 << 61) - 1, 3, modw(SECP_N)
    deals = []
    for i in range(6):
        D, V = (100, 500) if i % 2 == 0 else (512, 512)
        se = W([big(g, SECP_N) for _ in range(D)]) if i % 2 == 0 else g.words(D, PM)
        deals.append((i % 2 == 0, D, V, se, seed_block([g.seed() for _ in range(V)])))

    def run(p, s, sleep_cycles):
        with torch.cuda.stream(s):
            bufs = [(dev(se), dev(full((V, p.k, p.L, p.l))), dev(full((V, p.n, p.L, p.l)))) for _, D, V, se, _ in deals]
        torch.cuda.synchronize()
        if sleep_cycles:
            torch.cuda._sleep(sleep_cycles)                           # the current stream here is the legacy default stream
        t0 = time.perf_counter()
        for (wide, D, V, se, sd), (d_se, c1, c2) in zip(deals, bufs):
            if wide:
                p._call("pvw_deal_shares_wide_device", dptr(d_se), D, t, ptr(pw), 52, ptr(sd), dptr(c1), dptr(c2), N, sptr(s))
            else:
                p._call("pvw_deal_shares_device", dptr(d_se), D, t, PM, ptr(sd), dptr(c1), dptr(c2), N, sptr(s))
        s.synchronize()
        took = time.perf_counter() - t0
        torch.cuda.synchronize()
        return [(host(c1, np.uint64), host(c2, np.uint64)) for _, c1, c2 in bufs], took

    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    want, cold_s = run(ref, s, 0)                                     # the stream's first calls: allocations and the derived copies in front
    again, warm_s = run(ref, s, 0)
    assert not mismatches(again, want), "the twin's two serial runs differ"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cuda._sleep(50_000_000)
    torch.cuda.synchronize()
    per_s = 50_000_000 / (time.perf_counter() - t0)                   # sleep cycles a second
    # every attempt on a stream the context has never seen (a fresh workspace: r-hat and the share scratch are allocated and
    # zeroed again), the sleeps spread from 0.2 ms to past the end of the deals, so that some end while shares are in flight
    p, gpk, _ = context(geom, False)
    sleeps = [2e-4 + i * (1.5 * warm_s + 1e-3) / 16 for i in range(16)]
    bad = []
    for sleep_s in sleeps:
        got, took = run(p, torch.cuda.Stream(device=torch.device("cuda", 0)), int(sleep_s * per_s))
        bad += [(round(sleep_s * 1e3, 2), round(took * 1e3, 2), mismatches(got, want))] if mismatches(got, want) else []
    print(f"default-stream: six deals take {warm_s * 1e3:.1f} ms ({cold_s * 1e3:.1f} ms as a context's first calls); {len(sleeps)} attempts on fresh "
          f"streams while the default stream slept {sleeps[0] * 1e3:.1f} to {sleeps[-1] * 1e3:.1f} ms from their start", flush=True)
    assert not bad, ("deals enqueued while the default stream was busy differ from the serial ones: (sleep ms, took ms, deals)", bad)
    nz, scanned = api._secret_residue(p)
    print(f"default-stream: residue {nz} non-zero of {scanned} scanned words", flush=True)
    assert nz == 0 and scanned > 0, (nz, scanned)


CASES = {"cold": cold, "cold-bare": cold_bare, "mixed-plain": lambda: mixed("plain"), "mixed-packed56": lambda: mixed("packed56"), "staged": staged,
         "streams": streams, "rs": rs, "errors": errors}

if __name__ == "__main__":
    if sys.argv[1] == "selfcheck":
        selfcheck()
        sys.exit(0)
    selfcheck(whole=False)                                           # CPU only, before the GPU is touched
    assert torch.cuda.is_available()
    t0 = time.time()
    if {**CASES, "default-stream": default_stream}[sys.argv[1]]() is not False:
        print(f"{sys.argv[1]}: {time.time() - t0:.1f} s")
        print("WIDE_CONCURRENT_OK")

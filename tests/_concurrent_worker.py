"""Calls from several threads on ONE context (include/pvw_hip.h, Conventions): every host-buffer entry point, the
device-pointer calls on streams of their own, the _rs forms and deliberate argument errors, overlapping in time, bit for bit against
results computed serially on a TWIN context (same parameters, seeds and keys) and, where one exists, against ground truth -- the
dealt plaintexts, pvw_shamir_shares_host, pvw_shamir_reconstruct_checked_host, pvw_ct_sum_host, pvw_decode*_host,
pvw_wire_pack_host.  Every call has inputs of its own and sentinel-filled outputs; threads start each round from a barrier; a case
fails unless two calls from different threads did overlap; afterwards pvw_selftest_secret_residue reports nothing on the shared
context.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by
tests/test_gpu_concurrent_calls.py; prints CONCURRENT_OK (`selfcheck`: no GPU, prints CONCURRENT_SELFCHECK_OK)."""
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

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import EXAMPLE_MODULI, TEST_MODULI, decode_cases  # noqa: E402
from _staged_pieces_worker import all_layout, chunk, cut, passes  # noqa: E402  (the library's piece arithmetic, restated)

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
PM = (1 << 61) - 1
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)
SENTINEL = {np.dtype(np.uint64): MARK, np.dtype(np.uint32): np.uint32(0xA5A5A5A5), np.dtype(np.int64): np.int64(-0x5A5A5A5A5A5A5A5B),
            np.dtype(np.uint8): np.uint8(0xA5)}
THREADS = 8
STAGE_BYTES = 2048
ptr = api._ptr
GEOMS = {"packed56": (40, 64, 8, EXAMPLE_MODULI), "packed61": (40, 256, 8, M.bench_moduli(2)), "plain": (70, 12, 16, TEST_MODULI)}


# ---- comparison and overlap (checked without a GPU by `selfcheck`) ---------------------------------------------------------
def mismatches(got, want):
    """indices i where got[i] is missing or differs from want[i] (tuples of arrays) in count, dtype, shape or any bit"""
    bad = [i for i, (g, w) in enumerate(zip(got, want))
           if g is None or len(g) != len(w) or any(a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(g, w))]
    return bad + list(range(min(len(got), len(want)), max(len(got), len(want))))


def overlapping_pairs(spans):
    """spans: (thread, t0, t1) of every call of one round; pairs from DIFFERENT threads whose intervals intersect"""
    return sum(1 for a in range(len(spans)) for b in range(a + 1, len(spans))
               if spans[a][0] != spans[b][0] and spans[a][1] < spans[b][2] and spans[b][1] < spans[a][2])


def selfcheck():
    rng = np.random.default_rng(0)
    want = [(rng.integers(0, 1 << 63, (3, 4), dtype=np.uint64), rng.integers(0, 9, 5).astype(np.uint32)) for _ in range(6)]
    same = [tuple(a.copy() for a in w) for w in want]
    assert mismatches(same, want) == []
    swapped = list(same)
    swapped[1], swapped[4] = swapped[4], swapped[1]                 # a result handed to the wrong call
    assert mismatches(swapped, want) == [1, 4]
    flipped = [tuple(a.copy() for a in w) for w in want]
    flipped[2][0][2, 3] ^= np.uint64(1)                             # one bit
    assert mismatches(flipped, want) == [2]
    assert mismatches(same[:5] + [None], want) == [5] and mismatches(same[:4], want) == [4, 5]
    assert mismatches([(w[0], w[1].astype(np.uint64)) for w in want], want) == list(range(6))
    assert overlapping_pairs([(0, 0.0, 1.0), (1, 0.5, 1.5), (1, 2.0, 3.0), (0, 2.5, 2.6)]) == 2
    assert overlapping_pairs([(0, 0.0, 1.0), (0, 0.5, 1.5), (1, 1.5, 2.0)]) == 0      # same thread, and touching ends
    print("cases:", " ".join(sorted(CASES)))
    print("CONCURRENT_SELFCHECK_OK")


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def full(shape, dtype=np.uint64):
    return np.full(shape, SENTINEL[np.dtype(dtype)], dtype)


def dev(a):
    a = np.ascontiguousarray(a)
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view)).to(DEV)


def dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def sptr(s):
    return C.c_void_p(s.cuda_stream)


def seed_block(seeds):
    return np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()


def text(s):
    return np.frombuffer(s.encode(), dtype=np.uint8).copy()


class Gen:
    """inputs no other call has: one generator per (case, round)"""

    def __init__(self, *tag):
        self.rng = np.random.default_rng(list(tag))

    def seed(self):
        return self.rng.bytes(32)

    def words(self, shape, top=1 << 57):
        return self.rng.integers(0, top, shape, dtype=np.uint64)

    def residues(self, p, count):
        return np.ascontiguousarray(np.stack([self.rng.integers(0, q, (count, p.l), dtype=np.uint64) for q in p.moduli()], axis=1))


class Job:
    """one call (or one short sequence that belongs together) with inputs of its own: run(p, stream) -> tuple of arrays.
    truth: [(field, array)] the result must equal where the decode is proven exact; check(ref, want): a host restatement;
    want: preset expected values (calls that are not run on the twin)"""

    def __init__(self, name, run, truth=(), check=None, want=None, pieces=None):
        self.name, self.run, self.truth, self.check, self.want, self.pieces = name, run, list(truth), check, want, pieces


def context(geom, keys):
    n, k, l, moduli = GEOMS[geom]
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = None
    if keys:
        parties = [P.Party.new(i, p, SEED) for i in range(n)]
        gpk.generate_all_party_keys(parties, SEED)                  # pvw_keygen
    else:
        gpk.fill_uniform(SEED)
    return p, gpk, parties


class Dealt:
    """ciphertexts made beforehand (on the twin): D dealers' shares [D][n] below 2^57, in both representations, and every
    party's key"""

    def __init__(self, ref, gpk, parties, D=8):
        g = Gen(99, ref.n, ref.k)
        self.D = D
        self.shares = g.words((D, ref.n))
        cts = P.encrypt_many(self.shares.tolist(), gpk, [g.seed() for _ in range(D)], P.REPR_NTT)
        self.c1 = {P.REPR_NTT: np.stack([c.c1 for c in cts])}
        self.c2 = {P.REPR_NTT: np.stack([c.c2 for c in cts])}
        self.c1[P.REPR_POWER] = ref.ntt_inverse(self.c1[P.REPR_NTT]).reshape(self.c1[P.REPR_NTT].shape)
        self.c2[P.REPR_POWER] = ref.ntt_inverse(self.c2[P.REPR_NTT]).reshape(self.c2[P.REPR_NTT].shape)
        self.sk = np.ascontiguousarray(np.stack([api._i64(pt.secret_key.secret_coeffs) for pt in parties]))


# ---- the calls -------------------------------------------------------------------------------------------------------------
def j_encrypt(g, p0, repr=P.REPR_NTT, watch_error=False):
    seed, sc = g.seed(), g.words(p0.n, 1 << 32)

    def run(p, s):
        rnd, _ = api._randomness(p, seed, None, None, None)
        c1, c2 = full((p.k, p.L, p.l)), full((p.n, p.L, p.l))
        p._call("pvw_encrypt", ptr(sc), p.n, C.byref(rnd), ptr(c1), ptr(c2), repr)
        # a thread whose calls all succeed never sees another thread's message
        return (c1, c2, text(_ffi.last_error(p._lib))) if watch_error else (c1, c2)
    return Job("encrypt", run)


def j_multi(g, p0, D, repr=P.REPR_NTT):
    seeds, sc = seed_block([g.seed() for _ in range(D)]), g.words((D, p0.n), 1 << 32)
    item = (p0.k + p0.n) * p0.L * p0.l * 8 + p0.n * 8

    def run(p, s):
        c1, c2 = full((D, p.k, p.L, p.l)), full((D, p.n, p.L, p.l))
        p._call("pvw_encrypt_multi", ptr(sc), D, p.n, ptr(seeds), ptr(c1), ptr(c2), repr)
        return c1, c2
    return Job(f"encrypt_multi D={D}", run, pieces=lambda b: passes(item, D, b))


def j_batch(g, p0, dt, form, repr):
    i, d0 = int(g.rng.integers(0, p0.n)), int(g.rng.integers(0, 3))
    d1 = d0 + 4 + int(g.rng.integers(0, dt.D - d0 - 3))
    D = d1 - d0
    c1, col, sk = np.ascontiguousarray(dt.c1[repr][d0:d1]), np.ascontiguousarray(dt.c2[repr][d0:d1, i]), dt.sk[i]
    plain = dt.shares[d0:d1, i]

    def run(p, s):
        out, noise, status = full(D), full(D), full(D, np.uint32)
        head = (ptr(sk), ptr(c1), ptr(col), D, repr, ptr(out))
        if form == "values":
            nz = full((D, p.L, p.l))
            p._call("pvw_decrypt_batch", *head, ptr(nz))
            return out, nz
        if form == "checked":
            p._call("pvw_decrypt_batch_checked", *head, ptr(noise), ptr(status))
            return out, noise, status
        wide = full((D, 2))
        p._call("pvw_decrypt_batch_plain", *head, ptr(noise), ptr(status), PM, 2, ptr(wide))
        return out, noise, status, wide
    truth = [(0, plain % np.uint64(PM) if form == "plain" else plain)]
    return Job(f"decrypt_batch {form}", run, truth, pieces=lambda b: cut(D, chunk(p0.k * p0.L * p0.l * 8, D, b)))


def j_all(g, p0, dt, form, NP, repr):
    lo = int(g.rng.integers(0, p0.n - NP + 1))
    sel = np.sort(g.rng.choice(dt.D, 3 + int(g.rng.integers(0, 3)), replace=False))
    D = len(sel)
    c1, c2, sk = np.ascontiguousarray(dt.c1[repr][sel]), np.ascontiguousarray(dt.c2[repr][sel]), np.ascontiguousarray(dt.sk[lo:lo + NP])
    plain = np.ascontiguousarray(dt.shares[sel, lo:lo + NP].T)

    def run(p, s):
        out, noise, status = full((NP, D)), full((NP, D)), full((NP, D), np.uint32)
        head = (lo, lo + NP, ptr(sk), ptr(c1), ptr(c2), D, repr, ptr(out))
        if form == "values":
            p._call("pvw_decrypt_all", *head)
            return (out,)
        if form == "checked":
            p._call("pvw_decrypt_all_checked", *head, ptr(noise), ptr(status))
            return out, noise, status
        wide = full((NP, D, 2))
        p._call("pvw_decrypt_all_plain", *head, ptr(noise), ptr(status), PM, 2, ptr(wide))
        return out, noise, status, wide

    def pieces(b):
        lay = all_layout(p0, NP, D, True, True, b)
        return [(x, y) for x in cut(NP, lay["Pc"]) for y in cut(D, lay["Dg"])] if lay["gemm"] else cut(D, lay["Dc"])
    return Job(f"decrypt_all {form} P={NP}", run, [(0, plain % np.uint64(PM) if form == "plain" else plain)], pieces=pieces)


def _mask(g, D, masked):
    if not masked:
        return None, np.ones(D, bool)
    v = np.ones(D, np.uint8)
    v[g.rng.choice(D, 2, replace=False)] = 0
    return v, v != 0


def j_ct_sum(g, p0, dt, masked):
    repr = P.REPR_NTT
    valid, on = _mask(g, dt.D, masked)
    lo = int(g.rng.integers(0, 5)) if masked else 0
    hi = p0.n - int(g.rng.integers(0, 5)) if masked else p0.n
    c1s, c2s = dt.c1[repr], dt.c2[repr]

    def call(p, fn):
        c1, c2, cnt = full((p.k, p.L, p.l)), full((hi - lo, p.L, p.l)), C.c_uint32(77)
        p._call(fn, ptr(c1s), ptr(c2s), dt.D, ptr(valid), lo, hi, ptr(c1), ptr(c2), C.byref(cnt))
        return c1, c2, np.array([cnt.value], np.uint32)

    def check(ref, want):
        assert not mismatches([call(ref, "pvw_ct_sum_host")], [want]), "pvw_ct_sum_host"
    item = (p0.k + hi - lo) * p0.L * p0.l * 8
    return Job("ct_sum" + (" masked" if masked else ""), lambda p, s: call(p, "pvw_ct_sum"), check=check,
               pieces=lambda b: cut(int(on.sum()), chunk(item, int(on.sum()), b)))


def j_sum_checked(g, p0, dt, every, repr):
    valid, on = _mask(g, dt.D, True)
    c1s, c2s = dt.c1[repr], dt.c2[repr]
    nv = int(on.sum())
    if every:
        NP = 5 + int(g.rng.integers(0, 3))
        lo = int(g.rng.integers(0, p0.n - NP + 1))
        sk = np.ascontiguousarray(dt.sk[lo:lo + NP])
        plain = dt.shares[on][:, lo:lo + NP].sum(axis=0, dtype=np.uint64)

        def run(p, s):
            out, noise, status, cnt = full(NP), full(NP), full(NP, np.uint32), C.c_uint32(77)
            p._call("pvw_decrypt_all_sum_checked", lo, lo + NP, ptr(sk), ptr(c1s), ptr(c2s), dt.D, ptr(valid), repr, ptr(out), ptr(noise),
                    ptr(status), C.byref(cnt))
            return out, noise, status, np.array([cnt.value], np.uint32)
        item = (p0.k + NP) * p0.L * p0.l * 8
        return Job("decrypt_all_sum_checked", run, [(0, plain)], pieces=lambda b: cut(nv, chunk(item, nv, b)))
    i = int(g.rng.integers(0, p0.n))
    col, sk = np.ascontiguousarray(c2s[:, i]), dt.sk[i]
    plain = dt.shares[on][:, i].sum(dtype=np.uint64, keepdims=True)

    def run(p, s):
        out, noise, status, cnt = full(1), full(1), full(1, np.uint32), C.c_uint32(77)
        p._call("pvw_decrypt_sum_checked", ptr(sk), ptr(c1s), ptr(col), dt.D, ptr(valid), repr, ptr(out), ptr(noise), ptr(status), C.byref(cnt))
        return out, noise, status, np.array([cnt.value], np.uint32)
    item = (p0.k + 1) * p0.L * p0.l * 8
    return Job("decrypt_sum_checked", run, [(0, plain)], pieces=lambda b: cut(nv, chunk(item, nv, b)))


def j_shares(g, p0, D):
    t = 3 + int(g.rng.integers(0, 5))
    secrets, seeds = g.words(D, PM), seed_block([g.seed() for _ in range(D)])

    def call(p, fn):
        out = full((D, p.n))
        p._call(fn, ptr(secrets), D, t, PM, ptr(seeds), None, ptr(out))
        return (out,)

    def check(ref, want):
        assert not mismatches([call(ref, "pvw_shamir_shares_host")], [want]), "pvw_shamir_shares_host"
    return Job(f"shamir_shares D={D}", lambda p, s: call(p, "pvw_shamir_shares"), check=check,
               pieces=lambda b: cut(D, chunk((p0.n + 1) * 8, D, b)))


def j_deal(g, p0, D, repr=P.REPR_NTT):
    t = 2 + int(g.rng.integers(0, 6))
    secrets, seeds = g.words(D, PM), seed_block([g.seed() for _ in range(D)])
    item = (p0.k + p0.n) * p0.L * p0.l * 8 + 8

    def run(p, s):
        c1, c2 = full((D, p.k, p.L, p.l)), full((D, p.n, p.L, p.l))
        p._call("pvw_deal_shares", ptr(secrets), D, t, PM, ptr(seeds), ptr(c1), ptr(c2), repr)
        return c1, c2

    def check(ref, want):
        # the deal is pvw_encrypt_multi of the host shares under the same seeds
        sh = full((D, ref.n))
        ref._call("pvw_shamir_shares_host", ptr(secrets), D, t, PM, ptr(seeds), None, ptr(sh))
        c1, c2 = full((D, ref.k, ref.L, ref.l)), full((D, ref.n, ref.L, ref.l))
        ref._call("pvw_encrypt_multi", ptr(sh), D, ref.n, ptr(seeds), ptr(c1), ptr(c2), repr)
        assert not mismatches([(c1, c2)], [want]), "deal != encrypt_multi of the host shares"
    return Job(f"deal_shares D={D}", run, check=check, pieces=lambda b: passes(item, D, b))


def j_reconstruct(g, p0, degree, count, party_major):
    S = 3 + int(g.rng.integers(0, 4))
    secrets, seeds = g.words(S, PM), seed_block([g.seed() for _ in range(S)])
    idx = np.sort(g.rng.choice(p0.n, count, replace=False)).astype(np.uint64)
    sh = full((S, p0.n))
    p0._call("pvw_shamir_shares_host", ptr(secrets), S, degree, PM, ptr(seeds), None, ptr(sh))
    sh = np.ascontiguousarray(sh[:, idx.astype(np.int64)])
    bs, bc = int(g.rng.integers(0, S)), int(g.rng.integers(degree + 1, count))
    sh[bs, bc] = (sh[bs, bc] + np.uint64(1 + int(g.rng.integers(0, 1000)))) % np.uint64(PM)        # one deviating extra share
    arr = np.ascontiguousarray(sh.T) if party_major else sh
    strides = (1, S) if party_major else (count, 1)

    def call(p, fn, ctx=True):
        out, bad, col = full(S), full(S, np.uint32), full(count, np.uint32)
        args = (PM, degree, ptr(idx), count, ptr(arr), S, strides[0], strides[1], ptr(out), ptr(bad), ptr(col))
        if ctx:
            p._call(fn, *args)
        else:
            api._check(getattr(p._lib, fn)(*args), p._lib)
        return out, bad, col

    def check(ref, want):
        assert not mismatches([call(ref, "pvw_shamir_reconstruct_checked_host", False)], [want]), "pvw_shamir_reconstruct_checked_host"
        assert int(want[1][bs]) == 1 and int(want[2][bc]) == 1 and int(want[1].sum()) == 1
    return Job(f"reconstruct_checked ({degree}, {count}) {'party' if party_major else 'secret'}-major",
               lambda p, s: call(p, "pvw_shamir_reconstruct_checked"), [(0, secrets)], check)


def j_wire(g, p0):
    cnt = 3 + int(g.rng.integers(0, 6))
    polys = g.residues(p0, cnt)
    pb = p0.wire_poly_bytes()

    def run(p, s):
        data, back = full(cnt * pb, np.uint8), full(polys.shape)
        p._call("pvw_wire_pack", ptr(polys), cnt, ptr(data))
        p._call("pvw_wire_unpack", ptr(data), cnt, ptr(back))
        return data, back

    def check(ref, want):
        data = full(cnt * pb, np.uint8)
        ref._call("pvw_wire_pack_host", ptr(polys), cnt, ptr(data))
        assert np.array_equal(data, want[0]), "pvw_wire_pack_host"
    return Job("wire round trip", run, [(1, polys)], check)


_DECODE = {}


def decode_inputs(p0):
    key = (p0.l, tuple(p0.moduli()))
    if key not in _DECODE:
        cases = decode_cases(p0.l, p0.moduli())[::7]
        _DECODE[key] = np.ascontiguousarray(np.array([[[c % q for c in z] for q in p0.moduli()] for z in cases], dtype=np.uint64))
    return _DECODE[key]


def j_decode(g, p0, form):
    allz = decode_inputs(p0)
    nz = np.ascontiguousarray(allz[g.rng.choice(len(allz), 10, replace=False)])
    D = len(nz)

    def call(p, sfx):
        out, noise, status, wide = full(D), full(D), full(D, np.uint32), full((D, 2))
        if form == "values":
            p._call("pvw_decode" + sfx, ptr(nz), D, ptr(out))
            return (out,)
        if form == "checked":
            p._call("pvw_decode_checked" + sfx, ptr(nz), D, ptr(out), ptr(noise), ptr(status))
            return out, noise, status
        p._call("pvw_decode_plain" + sfx, ptr(nz), D, ptr(out), ptr(noise), ptr(status), PM, 2, ptr(wide))
        return out, noise, status, wide

    def check(ref, want):
        assert not mismatches([call(ref, "_host")], [want]), f"pvw_decode {form} host"
    return Job(f"decode {form}", lambda p, s: call(p, ""), check=check)


def j_ntt(g, p0, inverse):
    cnt = 4 + int(g.rng.integers(0, 8))
    polys = g.residues(p0, cnt)

    def run(p, s):
        a = polys.copy()
        p._call("pvw_ntt_inverse" if inverse else "pvw_ntt_forward", ptr(a), cnt)
        return (a,)

    def check(ref, want):
        b = want[0].copy()
        ref._call("pvw_ntt_forward" if inverse else "pvw_ntt_inverse", ptr(b), cnt)
        assert np.array_equal(b, polys), "the other transform does not give the input back"
    return Job("ntt inverse" if inverse else "ntt forward", run, check=check)


def j_sample(g, p0, kind):
    seed, index0, cnt = np.frombuffer(g.seed(), dtype=np.uint8).copy(), int(g.rng.integers(0, 1000)), 5 + int(g.rng.integers(0, 20))
    bound = 10 + int(g.rng.integers(0, 1 << 20))

    def run(p, s):
        if kind == "cbd":
            out = full((cnt, p.l), np.int64)
            p._call("pvw_sample_cbd", ptr(seed), _ffi.DOM_R, index0, cnt, 0.5, ptr(out))
        elif kind == "uniform":
            out = full((cnt, p.l), np.int64)
            p._call("pvw_sample_uniform", ptr(seed), _ffi.DOM_E1, index0, cnt, bound, ptr(out))
        else:
            out = full(cnt, np.int64)
            p._call("pvw_sample_gaussian", ptr(seed), index0, cnt, bound, ptr(out))
        return (out,)

    def check(ref, want):
        top = 1 if kind == "cbd" else bound
        assert int(np.abs(want[0]).max()) <= top and want[0].any(), kind
    return Job("sample " + kind, run, check=check)


def j_sk(g, p0, dt):
    """pvw_sk_load (on the context's own stream), pvw_decrypt_batch_device_sk on the calling thread's stream, pvw_sk_free"""
    i = int(g.rng.integers(0, p0.n))
    sel = np.sort(g.rng.choice(dt.D, 4, replace=False))
    c1, col, sk = dt.c1[P.REPR_NTT][sel], dt.c2[P.REPR_NTT][sel][:, i], dt.sk[i]
    D = len(sel)

    def run(p, s):
        h = C.c_void_p()
        p._call("pvw_sk_load", ptr(sk), C.byref(h))
        try:
            with torch.cuda.stream(s):
                d1, d2 = dev(c1), dev(col)
                nz, out = dev(full((D, p.L, p.l))), dev(full(D))
                p._call("pvw_decrypt_batch_device_sk", h, dptr(d1), dptr(d2), D, P.REPR_NTT, dptr(nz), dptr(out), sptr(s))
                s.synchronize()
                return (host(out, np.uint64),)
        finally:
            api._check(p._lib.pvw_sk_free(h), p._lib)
    return Job("sk_load + decrypt_batch_device_sk", run, [(0, dt.shares[sel, i])])


# device-pointer calls, each on the calling thread's stream
def j_encrypt_device(g, p0):
    seed, sc = g.seed(), g.words(p0.n, 1 << 32)

    def run(p, s):
        rnd, _ = api._randomness(p, seed, None, None, None)
        with torch.cuda.stream(s):
            d_sc, c1, c2 = dev(sc), dev(full((p.k, p.L, p.l))), dev(full((p.n, p.L, p.l)))
            p._call("pvw_encrypt_device", dptr(d_sc), p.n, C.byref(rnd), dptr(c1), dptr(c2), P.REPR_NTT, sptr(s))
            s.synchronize()
            return host(c1, np.uint64), host(c2, np.uint64)

    def check(ref, want):
        rnd, _ = api._randomness(ref, seed, None, None, None)
        c1, c2 = full((ref.k, ref.L, ref.l)), full((ref.n, ref.L, ref.l))
        ref._call("pvw_encrypt", ptr(sc), ref.n, C.byref(rnd), ptr(c1), ptr(c2), P.REPR_NTT)
        assert not mismatches([(c1, c2)], [want]), "pvw_encrypt_device != pvw_encrypt"
    return Job("encrypt_device", run, check=check)


def j_multi_device(g, p0, D):
    seeds, sc = seed_block([g.seed() for _ in range(D)]), g.words((D, p0.n), 1 << 32)

    def run(p, s):
        with torch.cuda.stream(s):
            d_sc, c1, c2 = dev(sc), dev(full((D, p.k, p.L, p.l))), dev(full((D, p.n, p.L, p.l)))
            p._call("pvw_encrypt_multi_device", dptr(d_sc), D, p.n, ptr(seeds), dptr(c1), dptr(c2), P.REPR_NTT, sptr(s))
            s.synchronize()
            return host(c1, np.uint64), host(c2, np.uint64)
    return Job(f"encrypt_multi_device D={D}", run)


def j_all_device(g, p0, dt, NP):
    lo = int(g.rng.integers(0, p0.n - NP + 1))
    sel = np.sort(g.rng.choice(dt.D, 4, replace=False))
    c1, c2, sk = dt.c1[P.REPR_NTT][sel], dt.c2[P.REPR_NTT][sel], dt.sk[lo:lo + NP]
    D = len(sel)

    def run(p, s):
        with torch.cuda.stream(s):
            d_sk, d1, d2, out = dev(sk), dev(c1), dev(c2), dev(full((NP, D)))
            p._call("pvw_decrypt_all_device", lo, lo + NP, dptr(d_sk), dptr(d1), dptr(d2), D, P.REPR_NTT, dptr(out), sptr(s))
            s.synchronize()
            return (host(out, np.uint64),)
    return Job(f"decrypt_all_device P={NP}", run, [(0, np.ascontiguousarray(dt.shares[sel, lo:lo + NP].T))])


def j_ct_sum_device(g, p0, dt, masked):
    valid, on = _mask(g, dt.D, masked)
    lo, hi = (2, p0.n - 3) if masked else (0, p0.n)
    c1s, c2s = dt.c1[P.REPR_NTT], dt.c2[P.REPR_NTT]

    def run(p, s):
        with torch.cuda.stream(s):
            d1, d2, dv = dev(c1s), dev(c2s), None if valid is None else dev(valid)
            o1, o2, cnt = dev(full((p.k, p.L, p.l))), dev(full((hi - lo, p.L, p.l))), dev(full(1, np.uint32))
            p._call("pvw_ct_sum_device", dptr(d1), dptr(d2), dt.D, dptr(dv), lo, hi, dptr(o1), dptr(o2), dptr(cnt), sptr(s))
            s.synchronize()
            return host(o1, np.uint64), host(o2, np.uint64), host(cnt, np.uint32)

    def check(ref, want):
        c1, c2, cnt = full((ref.k, ref.L, ref.l)), full((hi - lo, ref.L, ref.l)), C.c_uint32(77)
        ref._call("pvw_ct_sum_host", ptr(c1s), ptr(c2s), dt.D, ptr(valid), lo, hi, ptr(c1), ptr(c2), C.byref(cnt))
        assert not mismatches([(c1, c2, np.array([cnt.value], np.uint32))], [want]), "pvw_ct_sum_host"
    return Job("ct_sum_device", run, check=check)


# ---- running ---------------------------------------------------------------------------------------------------------------
def expected(ref, rounds, exact):
    """serially, on the twin: every job's values, held against its ground truth and its host restatement"""
    s = torch.cuda.Stream(device=DEV)
    want = []
    for jobs in rounds:
        row = []
        for j in jobs:
            w = j.want if j.want is not None else j.run(ref, s)
            assert all(not (a == SENTINEL[a.dtype]).all() for a in w if a.size > 2 and j.want is None), (j.name, "an output kept its sentinel")
            if j.check:
                j.check(ref, w)
            for field, value in j.truth:
                if exact:
                    assert np.array_equal(w[field], value), (j.name, "the serial result is not the ground truth", field)
            row.append(w)
        want.append(row)
    torch.cuda.synchronize()
    return want


def run_threads(p, rounds, plans, nthreads, streams=None):
    """rounds[r]: the jobs of round r; plans[r][t]: the indices thread t runs in round r, in order; streams[t]: the stream thread t
    owns.  All threads leave a barrier together at the start of every round.  Returns (got[r][i], spans[r], errors)."""
    streams = streams or [torch.cuda.Stream(device=DEV) for _ in range(nthreads)]
    torch.cuda.synchronize()
    got = [[None] * len(jobs) for jobs in rounds]
    spans = [[] for _ in rounds]
    errors = []
    barrier = threading.Barrier(nthreads)
    stop = threading.Event()

    def work(t):
        for r, jobs in enumerate(rounds):
            try:
                barrier.wait()
            except threading.BrokenBarrierError:
                return
            for i in plans[r][t]:
                if stop.is_set():
                    return
                try:
                    t0 = time.perf_counter()
                    res = jobs[i].run(p, streams[t])
                    t1 = time.perf_counter()
                except BaseException as e:                          # recorded; nothing more is started on the device
                    errors.append((r, t, jobs[i].name, repr(e)))
                    stop.set()
                    barrier.abort()
                    return
                got[r][i] = res
                spans[r].append((t, t0, t1))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    return got, spans, errors


def rotated_plans(rounds, nthreads, step=5):
    """round r hands the list, rotated by r * step, to the threads in turn: a thread alternates kinds, and a job kind moves to
    another thread (and so another recycled workspace) every round"""
    plans = []
    for r, jobs in enumerate(rounds):
        order = [(i + r * step) % len(jobs) for i in range(len(jobs))]
        plans.append([order[t::nthreads] for t in range(nthreads)])
    return plans


def finish(case, p, rounds, want, got, spans, errors, scanned_needed):
    assert not errors, ("a thread failed", errors)
    for r, jobs in enumerate(rounds):
        bad = mismatches(got[r], want[r])
        assert not bad, (case, "round", r, "calls whose results differ from the serial ones", [jobs[i].name for i in bad])
    pairs = [overlapping_pairs(s) for s in spans]
    print(f"{case}: {sum(len(s) for s in spans)} calls in {len(rounds)} rounds, overlapping call pairs per round {pairs}", flush=True)
    assert len(rounds) <= 5 and max(pairs) > 0, (case, "no two calls from different threads overlapped: the case proves nothing", pairs)
    nz, scanned = api._secret_residue(p)
    print(f"{case}: residue {nz} non-zero of {scanned} scanned words", flush=True)
    assert nz == 0 and (scanned > 0 or not scanned_needed), (case, "key material left on the device", nz, scanned)


def simple(case, geom, make_round, nrounds, keys, nthreads=THREADS, plans=None, scanned_needed=False, after=None):
    ref, ref_gpk, ref_parties = context(geom, keys)
    rounds = [make_round(ref, ref_gpk, ref_parties, r) for r in range(nrounds)]
    want = expected(ref, rounds, ref.sum_capacity() >= 8)
    p, gpk, parties = context(geom, keys)                           # the shared context: nothing but the loads has run on it
    got, spans, errors = run_threads(p, rounds, plans(rounds) if plans else rotated_plans(rounds, nthreads, 0), nthreads)
    finish(case, p, rounds, want, got, spans, errors, scanned_needed)
    if after:
        after(p, ref)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def cold_encrypt(geom):
    """8 threads make the context's FIRST pvw_encrypt calls together (no pvw_prepare, no warm-up: ensure_device's tail, the first
    workspaces and ensure_packed are entered while the threads overlap), then two more each"""
    width = {"packed56": 56, "packed61": 61}[geom]

    def make_round(ref, gpk, parties, r):
        g = Gen(1, r, width)
        return [j_encrypt(g, ref, P.REPR_POWER if (t + r) % 3 == 0 else P.REPR_NTT) for t in range(THREADS)]

    def after(p, ref):
        assert p.packed_active() == width, ("the packed stream did not run", p.packed_active())
        print(f"cold_encrypt {geom}: packed stream of {p.packed_active()} bits active", flush=True)
    simple(f"cold_encrypt {geom}", geom, make_round, 3, False, after=after)


def cold_multi():
    """the first calls are pvw_encrypt_multi with D = 2 (VALU) and D = 5 / 20 (matrix cores: ensure_xm and the GEMM buffers built
    concurrently), two pvw_encrypt threads among them"""
    def make_round(ref, gpk, parties, r):
        g = Gen(2, r)
        return [j_multi(g, ref, 2), j_multi(g, ref, 5), j_encrypt(g, ref), j_multi(g, ref, 20), j_multi(g, ref, 2), j_multi(g, ref, 5),
                j_encrypt(g, ref, P.REPR_POWER), j_multi(g, ref, 20, P.REPR_POWER)]

    def after(p, ref):
        assert p.packed_active() == 56 and p.derived_bytes()[1] > 0, (p.packed_active(), p.derived_bytes())
    simple("cold_multi packed56", "packed56", make_round, 3, False, after=after)


def mixed_round(ref, dt, r, tag, staged=False):
    """the job list of one round, kinds interleaved; staged: only the calls that stage host buffers, sized for >= 3 pieces"""
    g = Gen(tag, r, ref.n)
    N, W = P.REPR_NTT, P.REPR_POWER
    big = 40
    stage = [
        j_multi(g, ref, 9 if staged else 5), j_batch(g, ref, dt, "values", N), j_all(g, ref, dt, "checked", 5, N), j_ct_sum(g, ref, dt, False),
        j_deal(g, ref, 9 if staged else 6), j_sum_checked(g, ref, dt, False, N), j_all(g, ref, dt, "values", big, N), j_shares(g, ref, 7),
        j_batch(g, ref, dt, "plain", W), j_multi(g, ref, 12 if staged else 2, W), j_sum_checked(g, ref, dt, True, W), j_all(g, ref, dt, "plain", big, W),
        j_ct_sum(g, ref, dt, True), j_batch(g, ref, dt, "checked", N), j_deal(g, ref, 10 if staged else 2, W), j_all(g, ref, dt, "values", 5, W),
    ]
    if staged:
        return stage
    rest = [
        j_encrypt(g, ref), j_reconstruct(g, ref, 3, 9, False), j_wire(g, ref), j_decode(g, ref, "values"), j_ntt(g, ref, False),
        j_sample(g, ref, "cbd"), j_sk(g, ref, dt), j_encrypt(g, ref, W), j_reconstruct(g, ref, 5, 12, True), j_decode(g, ref, "checked"),
        j_ntt(g, ref, True), j_sample(g, ref, "uniform"), j_multi(g, ref, 3), j_decode(g, ref, "plain"), j_sample(g, ref, "gaussian"),
        j_encrypt(g, ref),
    ]
    return stage[:8] + rest[:8] + stage[8:] + rest[8:]              # thread t takes every 8th: staging and other kinds in turn


def mixed(geom):
    """keys from pvw_keygen, then 32 jobs of every kind per round on 8 threads, the list rotated from round to round: a recycled
    workspace goes to a call of another kind and size"""
    ref, ref_gpk, ref_parties = context(geom, True)
    dt = Dealt(ref, ref_gpk, ref_parties)
    rounds = [mixed_round(ref, dt, r, 3) for r in range(3)]
    exact = ref.sum_capacity() >= dt.D
    want = expected(ref, rounds, exact)
    print(f"mixed {geom}: decrypt results held against the dealt plaintexts: {exact} (sum_capacity {ref.sum_capacity()})", flush=True)
    p, gpk, parties = context(geom, True)
    got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS), THREADS)
    finish(f"mixed {geom}", p, rounds, want, got, spans, errors, True)


def staged():
    """the tuning build with a staging budget of 2048 bytes: every staging call of the mixed list takes three pieces or more, so a
    workspace is held across several copies while the other threads run; expected values: one piece each, on the twin"""
    if not os.path.exists(_ffi.LIB_TUNING_PATH):
        print("CONCURRENT_SKIP the tuning build is absent")
        return False
    _ffi.select("tuning")
    os.environ.pop("PVW_STAGE_BYTES", None)
    ref, ref_gpk, ref_parties = context("plain", True)
    assert ref._lib.pvw_build_is_tuning() == 1
    dt = Dealt(ref, ref_gpk, ref_parties)
    rounds = [mixed_round(ref, dt, r, 4, True) for r in range(3)]
    for j in rounds[0]:
        one, many = j.pieces(1 << 30), j.pieces(STAGE_BYTES)
        assert len(one) == 1 and len(many) >= 3, (j.name, one, many)
        print(f"staged {j.name}: pieces {many if len(many) < 12 else str(len(many)) + ' in all'}", flush=True)
    want = expected(ref, rounds, False)                              # one piece each
    p, gpk, parties = context("plain", True)
    os.environ["PVW_STAGE_BYTES"] = str(STAGE_BYTES)
    try:
        got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS), THREADS)
    finally:
        os.environ.pop("PVW_STAGE_BYTES", None)
    finish("staged plain", p, rounds, want, got, spans, errors, True)
    return True


def streams():
    """after pvw_prepare for each stream, 4 threads issue device-pointer calls on a stream of their own (the async_ws map under
    mu) while 2 threads make host-buffer calls (the pool)"""
    geom, T = "packed56", 6
    ref, ref_gpk, ref_parties = context(geom, True)
    dt = Dealt(ref, ref_gpk, ref_parties)

    def make_round(r):
        g = Gen(5, r)
        jobs, plan = [], []
        for t in range(4):
            kinds = [lambda: j_encrypt_device(g, ref), lambda: j_multi_device(g, ref, 5), lambda: j_all_device(g, ref, dt, 40 if t % 2 else 5),
                     lambda: j_ct_sum_device(g, ref, dt, t % 2 == 0)]
            mine = [kinds[(t + r + x) % 4]() for x in range(4)]
            plan.append(list(range(len(jobs), len(jobs) + len(mine))))
            jobs += mine
        for t in range(2):
            mine = [j_encrypt(g, ref), j_batch(g, ref, dt, "checked", P.REPR_NTT), j_ct_sum(g, ref, dt, True), j_multi(g, ref, 5)] if t == 0 else \
                   [j_all(g, ref, dt, "values", 5, P.REPR_NTT), j_deal(g, ref, 6), j_encrypt(g, ref, P.REPR_POWER), j_sum_checked(g, ref, dt, True, P.REPR_NTT)]
            plan.append(list(range(len(jobs), len(jobs) + len(mine))))
            jobs += mine
        return jobs, plan
    made = [make_round(r) for r in range(3)]
    rounds, plans = [m[0] for m in made], [m[1] for m in made]
    want = expected(ref, rounds, True)
    p, gpk, parties = context(geom, True)
    ss = [torch.cuda.Stream(device=DEV) for _ in range(T)]
    for s in ss[:4]:                                                # after this no device-pointer call on these streams allocates or builds
        p.prepare(_ffi.PREPARE_PACKED | _ffi.PREPARE_MFMA | _ffi.PREPARE_SUM, s.cuda_stream)
    got, spans, errors = run_threads(p, rounds, plans, T, ss)
    finish("streams packed56", p, rounds, want, got, spans, errors, True)


def rs():
    """every thread draws from a pvw_rnd_state of its own: 3 calls, equal to the seeded calls under call_seed(S, c + i); each
    counter ends where the serial count does"""
    geom = "packed56"
    ref, ref_gpk, _ = context(geom, False)
    p, gpk, _ = context(geom, False)
    Ds = [[1, 2, 1], [5, 1, 1], [1, 1, 5], [2, 1, 5], [1, 5, 2], [20, 1, 1], [1, 2, 2], [1, 1, 1]]     # 1: pvw_encrypt_rs; else multi_rs
    g = Gen(6)
    states, starts = [], []
    for t in range(THREADS):
        S, c = g.seed(), int(g.rng.integers(0, 1 << 40))
        states.append((S, P.DeviceRandomness(p, S, c)))
        starts.append(c)
    rounds, want = [], []
    cur = list(starts)
    for r in range(3):
        jobs, row = [], []
        for t in range(THREADS):
            D, (S, st) = Ds[t][r], states[t]
            sc = g.words((D, ref.n), 1 << 32)
            seeds = [P.DeviceRandomness.call_seed(S, cur[t] + d) for d in range(D)]
            cur[t] += D
            c1, c2 = full((D, ref.k, ref.L, ref.l)), full((D, ref.n, ref.L, ref.l))
            if D == 1:
                rnd, _ = api._randomness(ref, seeds[0], None, None, None)
                ref._call("pvw_encrypt", ptr(sc), ref.n, C.byref(rnd), ptr(c1), ptr(c2), P.REPR_NTT)
            else:
                ref._call("pvw_encrypt_multi", ptr(sc), D, ref.n, ptr(seed_block(seeds)), ptr(c1), ptr(c2), P.REPR_NTT)

            def run(q, s, D=D, sc=sc, st=st):
                o1, o2 = full((D, q.k, q.L, q.l)), full((D, q.n, q.L, q.l))
                if D == 1:
                    q._call("pvw_encrypt_rs", ptr(sc), q.n, st._h, ptr(o1), ptr(o2), P.REPR_NTT)
                else:
                    q._call("pvw_encrypt_multi_rs", ptr(sc), D, q.n, st._h, ptr(o1), ptr(o2), P.REPR_NTT)
                return o1, o2
            jobs.append(Job(f"encrypt_rs D={D}", run, want=(c1, c2)))
            row.append((c1, c2))
        rounds.append(jobs)
        want.append(row)
    got, spans, errors = run_threads(p, rounds, rotated_plans(rounds, THREADS, 0), THREADS)
    finish("rs packed56", p, rounds, want, got, spans, errors, False)
    ends = [st.counter() for _, st in states]
    assert ends == cur, ("counters", ends, cur)
    for _, st in states:
        st.free()
    print(f"rs: counters advanced by {[e - s for e, s in zip(ends, starts)]}", flush=True)


def errors():
    """one thread makes calls that are refused for their arguments (before any launch) while seven encrypt: the refused calls get
    their code and message every time, the encrypts are exact, and no succeeding thread's pvw_last_error shows another's text"""
    geom = "packed56"
    ref, _, _ = context(geom, False)
    n, k = ref.n, ref.k
    sc, seeds = np.zeros((2, n), np.uint64), np.zeros(64, np.uint8)
    expect = [(1, "NULL argument"), (1, f"Party index {n + 2} exceeds maximum {n - 1}"), (1, "no dealers")] * 40

    def refused(p, s):
        rnd, _ = api._randomness(p, SEED, None, None, None)
        c1, c2 = full((2, k, p.L, p.l)), full((2, n, p.L, p.l))
        sk, out = np.zeros((5, k, p.l), np.int64), full((5, 2))
        lib, seen = p._lib, []
        for x in range(40):
            for call in (lambda: lib.pvw_encrypt(p._h, ptr(sc), n, C.byref(rnd), None, ptr(c2), P.REPR_NTT),              # NULL output
                         lambda: lib.pvw_decrypt_all(p._h, n - 2, n + 3, ptr(sk), ptr(c1), ptr(c2), 2, P.REPR_NTT, ptr(out)),   # parties the context does not have
                         lambda: lib.pvw_encrypt_multi(p._h, ptr(sc), 0, n, ptr(seeds), ptr(c1), ptr(c2), P.REPR_NTT)):         # D = 0
                rc = call()
                seen.append((rc, _ffi.last_error(lib)))
        assert (c1 == MARK).all() and (c2 == MARK).all() and (out == MARK).all(), "a refused call wrote to its outputs"
        return np.array([rc for rc, _ in seen], np.int32), text("|".join(m for _, m in seen))
    want_refused = (np.array([rc for rc, _ in expect], np.int32), text("|".join(m for _, m in expect)))

    def make_round(ref_, gpk, parties, r):
        g = Gen(7, r)
        return [Job("refused calls", refused, want=want_refused)] + [j_encrypt(g, ref_, watch_error=True) for _ in range(2 * (THREADS - 1))]
    # thread 0 makes the refused calls, every other thread two encrypts
    plans = lambda rounds: [[[0]] + [[2 * t - 1, 2 * t] for t in range(1, THREADS)] for _ in rounds]
    simple("errors packed56", geom, make_round, 3, False, plans=plans)


CASES = {"cold_encrypt-packed56": lambda: cold_encrypt("packed56"), "cold_encrypt-packed61": lambda: cold_encrypt("packed61"),
         "cold_multi": cold_multi, "mixed-packed56": lambda: mixed("packed56"), "mixed-plain": lambda: mixed("plain"), "staged": staged,
         "streams": streams, "rs": rs, "errors": errors}

if __name__ == "__main__":
    if sys.argv[1] == "selfcheck":
        selfcheck()
        sys.exit(0)
    selfcheck()                                                     # CPU only, before the GPU is touched
    assert torch.cuda.is_available()
    t0 = time.time()
    if CASES[sys.argv[1]]() is not False:
        print(f"{sys.argv[1]}: {time.time() - t0:.1f} s")
        print("CONCURRENT_OK")

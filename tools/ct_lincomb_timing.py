#!/usr/bin/env python3
"""Weighted sums of dealers' ciphertexts against the plain sum on the same bytes and against what a caller did
before them, interleaved in one process on one stream (run on the GPU box, every step under a time limit of its own, chained,
nothing tried twice):
    timeout -k 10 300 python tools/ct_lincomb_timing.py --only kernel && timeout -k 10 300 python tools/ct_lincomb_timing.py --only all
    [--rounds 7] [--steps 10] [--tuning]
One JSON line per case; every figure is the median over the rounds of the mean of --steps calls between two HIP events
(kernel figures: the library's own event pairs, pvw_ctx_kernel_time).  Uniform random words, after pvw_prepare(PVW_PREPARE_SUM).
  kernel      ct_lincomb against ct_sum on the SAME buffers (the bytes are the same, so the existing kernel is the yardstick):
              config-5 shard (D = 1024, k = 512, l = 16, 34 moduli, column form) and config 3 (k = 256, l = 8, 17 moduli,
              D = 1024 whole rows of n = 4096); weights small (|w| < 8: the residue is a compare), centred in a 61-bit field
              (the handover: most lanes reduce) and uniform int64 (every lane reduces); the ratio to ct_sum with ct_sum's own
              round-to-round spread beside it; every kernel row carries its share of the 8.0 TB/s datasheet peak (of_peak, comparable
              with profiles/r05_ct_sum.txt) AND of the 6.3 TB/s a streaming copy achieves (of_achievable, DESIGN 8.12's yardstick)
  all         pvw_decrypt_all_lincomb_plain_device against pvw_decrypt_all_plain_device plus the combine of its [P][D] result in
              torch (mod 2^61 - 1), at P = D = 1024, config 3, with the kernel times of the former"""
import ctypes as C
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: E402

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402

dev = torch.device("cuda", 0)
PEAK = 8.0e12         # the HBM3E datasheet peak, as tools/ct_sum_timing.py: `of_peak`
ACHIEVABLE = 6.3e12   # what a streaming copy reaches on this part, the figure DESIGN 8.12 argues with: `of_achievable`
PLAIN = (1 << 61) - 1


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rand(*shape):
    return torch.empty(shape, dtype=torch.int64, device=dev).random_()


def timed(fn, steps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, steps, rounds, stream):
    """median ms per call of each fn, the order alternating from round to round"""
    for fn in fns:
        timed(fn, 2, stream)
    acc = [[] for _ in fns]
    for r in range(rounds):
        order = list(range(len(fns)))
        if r % 2:
            order.reverse()
        for i in order:
            acc[i].append(timed(fns[i], steps, stream))
    return [float(np.median(a)) for a in acc], [[round(x, 4) for x in a] for a in acc]


def kernel_ms(p, fn, names, steps, stream):
    """per call: the library's event-pair time of each named kernel scope"""
    p.set_profiling(True)
    p.reset_profiling()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    out = {nm: round(p.kernel_time(nm)[0] / steps, 4) for nm in names}
    p.set_profiling(False)
    return out


def params(n, k, l, L):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(M.bench_moduli(L)).build()


def emit(**kw):
    print(json.dumps(dict(kw, host=socket.gethostname())), flush=True)


def weights(kind, D):
    rng = np.random.default_rng(D)
    if kind == "small":
        w = rng.integers(1, 8, D, dtype=np.int64) * rng.choice(np.array([-1, 1], np.int64), D)
    elif kind == "field":
        w = rng.integers(-(PLAIN // 2), PLAIN // 2, D, dtype=np.int64, endpoint=True)
        w[w == 0] = 1
    else:
        w = rng.integers(-(1 << 63), (1 << 63) - 1, D, dtype=np.int64, endpoint=True)
        w[w == 0] = 1
    return torch.from_numpy(w).to(dev)


def kernel_case(name, n, k, l, L, D, rows, steps, rounds, s):
    p = params(n, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    o1, o2 = rand(k, L, l), rand(rows, L, l)
    kinds = ("small", "field", "int64")
    w = {kind: weights(kind, D) for kind in kinds}
    plain = lambda: p._call("pvw_ct_sum_device", ptr(c1), ptr(c2), D, None, 0, rows, ptr(o1), ptr(o2), None, sp)          # noqa: E731
    comb = {kind: (lambda kind=kind: p._call("pvw_ct_lincomb_device", ptr(c1), ptr(c2), D, None, ptr(w[kind]), 0, rows, ptr(o1),
                                             ptr(o2), None, sp)) for kind in kinds}
    order0 = [("ct_sum", plain, "ct_sum")] + [("ct_lincomb_" + kind, comb[kind], "ct_lincomb") for kind in kinds]
    for _, fn, _ in order0:
        timed(fn, 2, s)
    acc = {key: [] for key, _, _ in order0}
    for r in range(rounds):
        order = list(order0)
        if r % 2:
            order.reverse()
        for key, fn, scope in order:
            acc[key].append(kernel_ms(p, fn, [scope], steps, s)[scope])
    by = 8 * L * l * (D + 1) * (k + rows)
    res = {}
    for key, v in acc.items():
        ms = float(np.median(v))
        res[key] = {"ms": round(ms, 4), "rounds_ms": v, "TBps": round(by / ms / 1e9, 3), "of_peak": round(by / ms / 1e9 / (PEAK / 1e12), 3),
                    "of_achievable": round(by / ms / 1e9 / (ACHIEVABLE / 1e12), 3)}
    base = res["ct_sum"]
    spread = round((max(base["rounds_ms"]) - min(base["rounds_ms"])) / base["ms"], 4)
    ratios = {key: round(res[key]["ms"] / base["ms"], 4) for key in res if key != "ct_sum"}
    emit(case="kernel " + name, n=n, k=k, l=l, L=L, dealers=D, rows=rows, steps=steps, rounds=rounds, bytes=by, ct_sum_spread=spread,
         ratio_to_ct_sum=ratios, **res)


def mulmod61(x, w):
    """x * w mod 2^61 - 1 for tensors of values below 2^61, in int64 arithmetic (2^61 = 1 mod p)"""
    m31, m30 = (1 << 31) - 1, (1 << 30) - 1
    xl, xh, wl, wh = x & m31, x >> 31, w & m31, w >> 31

    def fold(v):                                                  # v < 2^63: v mod p
        v = (v & PLAIN) + (v >> 61)
        return torch.where(v >= PLAIN, v - PLAIN, v)

    def shift31(v):                                               # v < 2^61: v * 2^31 mod p
        return fold(((v & m30) << 31) + (v >> 30))

    hh = fold(xh * wh)                                            # weight 2^62 = 2 mod p
    mid = fold(fold(xh * wl) + fold(xl * wh))
    return fold(fold(fold(hh + hh) + shift31(mid)) + fold(xl * wl))


def combine61(vals, w):
    """sum_d w[d] * vals[:, d] mod 2^61 - 1, w as residues: [P]"""
    t = mulmod61(vals, w[None, :])
    lo, hi = (t & ((1 << 31) - 1)).sum(dim=1), (t >> 31).sum(dim=1)    # D < 2^30 terms
    v = lo + ((hi & ((1 << 30) - 1)) << 31) + (hi >> 30)
    v = (v & PLAIN) + (v >> 61)
    return torch.where(v >= PLAIN, v - PLAIN, v)


def all_case(NP, steps, rounds, s):
    n, k, l, L = 4096, 256, 8, 17
    D = NP
    p = params(n, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    sk = torch.randint(-1, 2, (NP, k, l), dtype=torch.int64, device=dev)
    w = weights("field", D)
    wres = torch.where(w < 0, w + PLAIN, w)
    out, ns, st = rand(NP, D), rand(NP, D), torch.zeros((NP, D), dtype=torch.int32, device=dev)
    o1, n1, s1 = rand(NP), rand(NP), torch.zeros(NP, dtype=torch.int32, device=dev)

    def before():
        p._call("pvw_decrypt_all_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, P.REPR_NTT, ptr(out), ptr(ns), ptr(st), PLAIN, 0, None, sp)
        return combine61(out, wres)

    after = lambda: p._call("pvw_decrypt_all_lincomb_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, None, ptr(w), P.REPR_NTT, ptr(o1),  # noqa: E731
                            ptr(n1), ptr(s1), None, PLAIN, 0, None, sp)
    (ms_before, ms_after), rr = interleaved([before, after], steps, rounds, s)
    parts = kernel_ms(p, after, ["ct_lincomb", "prep", "digits", "gemm", "finish", "decrypt_mac", "intt", "decode"], steps, s)
    emit(case="all", parties=NP, dealers=D, n=n, k=k, l=l, L=L, steps=steps, rounds=rounds, ms_decrypt_all_plus_combine=round(ms_before, 4),
         ms_decrypt_all_lincomb=round(ms_after, 4), speedup=round(ms_before / ms_after, 2), before_rounds_ms=rr[0], lincomb_rounds_ms=rr[1],
         lincomb_kernels_ms=parts)


def main():
    rounds, steps = int(arg("--rounds", 7)), int(arg("--steps", 10))
    only = arg("--only", "")
    if "--tuning" in sys.argv:              # the measurement build: PVW_SUM_SPLIT selects the kernel form
        from pvw_rs_amd import _ffi
        _ffi.select("tuning")
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        if only in ("", "kernel"):
            kernel_case("config-5 shard, column form", 1, 512, 16, 34, 1024, 1, steps, rounds, s)
            kernel_case("config 3, whole rows", 4096, 256, 8, 17, 1024, 4096, max(steps // 2, 2), rounds, s)
        if only in ("", "all"):
            all_case(1024, max(steps // 3, 2), rounds, s)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Sums of dealers' ciphertexts against what a caller did before them, interleaved in one process on one stream
(run on the GPU box):
    python tools/ct_sum_timing.py [--rounds 7] [--steps 10] [--only kernel|party|all] [--tuning]
One JSON line per case; every figure is the median over the rounds of the mean of --steps calls between two HIP events
(kernel figures: the library's own event pairs, pvw_ctx_kernel_time).  Uniform random words, after pvw_prepare(PVW_PREPARE_SUM).
  kernel      ct_sum alone against decrypt_mac (the full-width form) on the SAME buffers: config-5 shard (D = 1024, k = 512,
              l = 16, 34 moduli, column form) and config 3 (k = 256, l = 8, 17 moduli; D = 1024 whole rows of n = 4096 for the
              sum, its c1 for decrypt_mac); algorithmic bytes 8 L l (D_valid + 1) (k + R), fraction of 8 TB/s; again with half
              the dealers masked out
  party       pvw_decrypt_sum_device_sk_checked against pvw_decrypt_batch_device_sk_checked over the D dealers
              (config-5 shard D = 1024; the d3 geometry k = 256, l = 8, 17 moduli, D = 2048)
  all         pvw_decrypt_all_sum_checked_device against pvw_decrypt_all_checked_device at P = D in {64, 256, 1024}, config 3,
              with the sum / product / decode kernel times of the former"""
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
PEAK = 8.0e12


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


def kernel_case(name, n, k, l, L, D, rows, steps, rounds, s):
    p = params(n, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    o1, o2 = rand(k, L, l), rand(rows, L, l)
    sk, nz = torch.randint(-1, 2, (k, l), dtype=torch.int64, device=dev), rand(D, L, l)
    col = c2[:, 0].contiguous()
    half = torch.from_numpy((np.arange(D) % 2).astype(np.uint8)).to(dev)
    sum_all = lambda: p._call("pvw_ct_sum_device", ptr(c1), ptr(c2), D, None, 0, rows, ptr(o1), ptr(o2), None, sp)       # noqa: E731
    sum_half = lambda: p._call("pvw_ct_sum_device", ptr(c1), ptr(c2), D, ptr(half), 0, rows, ptr(o1), ptr(o2), None, sp)  # noqa: E731
    mac = lambda: p._call("pvw_decrypt_noisy_device", ptr(sk), ptr(c1), ptr(col), D, P.REPR_NTT, ptr(nz), sp)             # noqa: E731
    for fn in (sum_all, sum_half, mac):
        timed(fn, 2, s)
    acc = {"ct_sum": [], "ct_sum_half": [], "decrypt_mac": []}
    for r in range(rounds):
        order = [("ct_sum", sum_all, "ct_sum"), ("ct_sum_half", sum_half, "ct_sum"), ("decrypt_mac", mac, "decrypt_mac")]
        if r % 2:
            order.reverse()
        for key, fn, scope in order:
            acc[key].append(kernel_ms(p, fn, [scope], steps, s)[scope])
    P8 = 8 * L * l
    by = {"ct_sum": P8 * (D + 1) * (k + rows), "ct_sum_half": P8 * (D // 2 + 1) * (k + rows), "decrypt_mac": P8 * (D * (k + 2) + k)}
    res = {}
    for key, v in acc.items():
        ms = float(np.median(v))
        res[key] = {"ms": round(ms, 4), "rounds_ms": v, "bytes": by[key], "TBps": round(by[key] / ms / 1e9, 3),
                    "of_peak": round(by[key] / ms / 1e9 / (PEAK / 1e12), 3)}
    emit(case="kernel " + name, n=n, k=k, l=l, L=L, dealers=D, rows=rows, steps=steps, rounds=rounds, **res)


def party_case(name, k, l, L, D, steps, rounds, s):
    p = params(2, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    sp = C.c_void_p(s.cuda_stream)
    c1, col = rand(D, k, L, l), rand(D, L, l)
    nz, out, ns = rand(D, L, l), rand(D), rand(D)
    st = torch.zeros(D, dtype=torch.int32, device=dev)
    key = P.DeviceSecretKey(P.SecretKey(p, np.random.default_rng(1).integers(-1, 2, (k, l), dtype=np.int64)))
    batch = lambda: p._call("pvw_decrypt_batch_device_sk_checked", key._h, ptr(c1), ptr(col), D, P.REPR_NTT, ptr(nz), ptr(out), ptr(ns),  # noqa: E731
                            ptr(st), sp)
    total = lambda: key.decrypt_sum_device_checked(c1, col, D, out, d_noise=ns, d_status=st, stream=s)                   # noqa: E731
    (ms_batch, ms_sum), rr = interleaved([batch, total], steps, rounds, s)
    parts = kernel_ms(p, total, ["ct_sum", "decrypt_mac", "intt", "decode"], steps, s)
    emit(case="party " + name, k=k, l=l, L=L, dealers=D, steps=steps, rounds=rounds, ms_decrypt_batch=round(ms_batch, 4),
         ms_decrypt_sum=round(ms_sum, 4), speedup=round(ms_batch / ms_sum, 2), batch_rounds_ms=rr[0], sum_rounds_ms=rr[1],
         sum_kernels_ms=parts)
    key.free()


def all_case(NP, steps, rounds, s):
    n, k, l, L = 4096, 256, 8, 17
    D = NP
    p = params(n, k, l, L)
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    sk = torch.randint(-1, 2, (NP, k, l), dtype=torch.int64, device=dev)
    out, ns, st = rand(NP, D), rand(NP, D), torch.zeros((NP, D), dtype=torch.int32, device=dev)
    full = lambda: p._call("pvw_decrypt_all_checked_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, P.REPR_NTT, ptr(out), ptr(ns), ptr(st), sp)  # noqa: E731
    summed = lambda: p._call("pvw_decrypt_all_sum_checked_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, None, P.REPR_NTT, ptr(out),          # noqa: E731
                             ptr(ns), ptr(st), None, sp)
    (ms_full, ms_sum), rr = interleaved([full, summed], steps, rounds, s)
    parts = kernel_ms(p, summed, ["ct_sum", "prep", "digits", "gemm", "finish", "decrypt_mac", "intt", "decode"], steps, s)
    emit(case="all", parties=NP, dealers=D, n=n, k=k, l=l, L=L, steps=steps, rounds=rounds, ms_decrypt_all=round(ms_full, 4),
         ms_decrypt_all_sum=round(ms_sum, 4), speedup=round(ms_full / ms_sum, 2), all_rounds_ms=rr[0], sum_rounds_ms=rr[1],
         sum_kernels_ms=parts)


def main():
    rounds, steps = int(arg("--rounds", 7)), int(arg("--steps", 10))
    only = arg("--only", "")
    if "--tuning" in sys.argv:              # the measurement build: PVW_SUM_SPLIT / PVW_SUM_U select the kernel form
        from pvw_rs_amd import _ffi
        _ffi.select("tuning")
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        if only in ("", "kernel"):
            kernel_case("config-5 shard, column form", 1, 512, 16, 34, 1024, 1, steps, rounds, s)
            kernel_case("config 3, whole rows", 4096, 256, 8, 17, 1024, 4096, max(steps // 2, 2), rounds, s)
        if only in ("", "party"):
            party_case("config-5 shard", 512, 16, 34, 1024, steps, rounds, s)
            party_case("d3", 256, 8, 17, 2048, steps, rounds, s)
        if only in ("", "all"):
            for NP in (64, 256, 1024):
                all_case(NP, max(steps // 3, 2), rounds, s)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Corrected Shamir reconstruction on the device beside the checked call it extends, in one process (run on the
GPU box):
    python tools/correct_timing.py [--steps 3] [--rounds 5]
pvw_shamir_reconstruct_corrected_device on one stream, on shares made by pvw_shamir_shares_device, n = 4096, t = 2047 (r = 2048,
E = 1024), p = 2^61 - 1, at S = 64 and S = 1024, once on the consistent sharing (every syndrome 0: Berlekamp-Massey does no update
and no atomic is issued) and once with 1024 whole columns overwritten (every row at the correction bound):
  call      the whole call between two HIP events, --steps calls back to back, after warm-up
  weights   the points, products and the two public matrices, from the context's profiling scope shamir_correct_weights
  decode    syndromes, Berlekamp-Massey, locator values and the finish kernel (scope shamir_correct)
  checked   pvw_shamir_reconstruct_checked_device on the same input, as a whole: what existed before; on the overwritten input
            its secrets are wrong
One JSON line per shape and input: median ms over the rounds."""
import ctypes as C
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: E402

import pvw_rs_amd as P  # noqa: E402

dev = torch.device("cuda", 0)
P61 = (1 << 61) - 1
MODULI = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn, steps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    steps, rounds = int(arg("--steps", 3)), int(arg("--rounds", 5))
    n, t, Smax = 4096, 2047, 1024
    E = (n - t - 1) // 2
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rng = np.random.default_rng(1)
    secrets = rng.integers(0, P61, size=Smax, dtype=np.uint64)
    d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
    seeds = rng.integers(0, 256, size=Smax * 32, dtype=np.uint8)
    clean = torch.empty((Smax, n), dtype=torch.int64, device=dev)
    P.api._check(lib.pvw_shamir_shares_device(p._h, ptr(d_se), Smax, t, P61, seeds.ctypes.data_as(C.c_void_p), None, ptr(clean), sp), lib)
    s.synchronize()
    planted = np.sort(rng.choice(n, size=E, replace=False))
    bent = clean.clone()
    junk = torch.from_numpy(rng.integers(1, P61, size=(Smax, E), dtype=np.int64)).to(dev)
    bent[:, planted] = (bent[:, planted] + junk) % P61
    ix = np.arange(n, dtype=np.uint64)
    ixp = ix.ctypes.data_as(C.c_void_p)
    out = torch.empty(Smax, dtype=torch.int64, device=dev)
    nerr = torch.empty(Smax, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty((Smax, n // 64), dtype=torch.int64, device=dev)
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    for S in (64, Smax):
        for name, shares, want_err in (("consistent", clean, 0), ("at_the_bound", bent, E)):
            call = lambda: P.api._check(lib.pvw_shamir_reconstruct_corrected_device(p._h, P61, t, ixp, n, ptr(shares), S, n, 1, ptr(out),  # noqa: E731
                                                                                    ptr(nerr), ptr(col), ptr(mask), sp), lib)
            old = lambda: P.api._check(lib.pvw_shamir_reconstruct_checked_device(p._h, P61, t, ixp, n, ptr(shares), S, n, 1, ptr(out),  # noqa: E731
                                                                                 ptr(nerr), ptr(col), sp), lib)
            timed(call, 1, s)                                       # warm-up (sizes the workspace)
            ok = bool((out[:S].cpu().numpy().view(np.uint64) == secrets[:S]).all()) and bool((nerr[:S] == want_err).all().item())
            whole = [timed(call, steps, s) for _ in range(rounds)]
            wts, dec = [], []
            p.set_profiling(True)
            for _ in range(rounds):
                p.reset_profiling()
                timed(call, steps, s)
                wts.append(p.kernel_time("shamir_correct_weights")[0] / steps)
                dec.append(p.kernel_time("shamir_correct")[0] / steps)
            p.set_profiling(False)
            timed(old, 1, s)
            chk = [timed(old, steps, s) for _ in range(rounds)]
            print(json.dumps({"S": S, "count": n, "degree": t, "input": name, "steps": steps, "rounds": rounds, "correct": ok,
                              "ms_call": med(whole), "ms_weights": med(wts), "ms_decode": med(dec), "ms_checked_call": med(chk),
                              "rounds_ms": {"call": [round(x, 4) for x in whole], "weights": [round(x, 4) for x in wts],
                                            "decode": [round(x, 4) for x in dec], "checked": [round(x, 4) for x in chk]},
                              "host": socket.gethostname()}), flush=True)


if __name__ == "__main__":
    main()

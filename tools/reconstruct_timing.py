#!/usr/bin/env python3
"""Checked Shamir reconstruction on the device against the host reconstruction it extends, in one process (run
on the GPU box):
    python tools/reconstruct_timing.py [--steps 5] [--rounds 5]
pvw_shamir_reconstruct_checked_device on one stream, on shares made by pvw_shamir_shares_device (a consistent sharing: nothing
deviates, so no atomic is issued), at (S, count, t) = (8192, 4096, 2047), (8192, 2049, 2047) and (64, 4096, 2047), p = 2^61 - 1:
  call      the whole call between two HIP events, --steps calls back to back, after warm-up
  weights   the points and shamir_weights_kernel (with its product pass), from the context's profiling scopes
  interp    shamir_interp_kernel (with the kernel that clears bad), likewise; profiling is switched on for rounds of its own
  host      wall time of the host pvw_shamir_reconstruct on the first t + 1 columns of the same input: what existed before,
            and it checks nothing
One JSON line per shape: median ms over the rounds."""
import ctypes as C
import json
import os
import socket
import sys
import time

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
    steps, rounds = int(arg("--steps", 5)), int(arg("--rounds", 5))
    n, t, Smax = 4096, 2047, 8192
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rng = np.random.default_rng(1)
    secrets = rng.integers(0, P61, size=Smax, dtype=np.uint64)
    d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
    seeds = rng.integers(0, 256, size=Smax * 32, dtype=np.uint8)
    shares = torch.empty((Smax, n), dtype=torch.int64, device=dev)
    P.api._check(lib.pvw_shamir_shares_device(p._h, ptr(d_se), Smax, t, P61, seeds.ctypes.data_as(C.c_void_p), None, ptr(shares), sp), lib)
    s.synchronize()
    h_shares = shares.cpu().numpy().view(np.uint64)
    ix = np.arange(n, dtype=np.uint64)
    ixp = ix.ctypes.data_as(C.c_void_p)
    out = torch.empty(Smax, dtype=torch.int64, device=dev)
    bad = torch.empty(Smax, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    for S, count in ((8192, 4096), (8192, 2049), (64, 4096)):
        call = lambda: P.api._check(lib.pvw_shamir_reconstruct_checked_device(p._h, P61, t, ixp, count, ptr(shares), S, n, 1, ptr(out), ptr(bad),  # noqa: E731
                                                                              ptr(col), sp), lib)
        timed(call, 2, s)                                       # warm-up (sizes the workspace)
        ok = bool((out[:S].cpu().numpy().view(np.uint64) == secrets[:S]).all()) and not bad[:S].any().item() and not col[:count].any().item()
        whole = [timed(call, steps, s) for _ in range(rounds)]
        wts, itp = [], []
        p.set_profiling(True)
        for _ in range(rounds):
            p.reset_profiling()
            timed(call, steps, s)
            wts.append(p.kernel_time("shamir_weights")[0] / steps)
            itp.append(p.kernel_time("shamir_interp")[0] / steps)
        p.set_profiling(False)
        # the host routine on the basis columns alone
        basis = np.ascontiguousarray(h_shares[:S, :t + 1])
        h_out = np.zeros(S, dtype=np.uint64)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            P.api._check(lib.pvw_shamir_reconstruct(P61, ixp, basis.ctypes.data_as(C.c_void_p), t + 1, S, h_out.ctypes.data_as(C.c_void_p)), lib)
            host.append((time.perf_counter() - t0) * 1e3)
        ok = ok and bool((h_out == secrets[:S]).all())
        T = count - t
        med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
        print(json.dumps({"S": S, "count": count, "degree": t, "steps": steps, "rounds": rounds, "correct": ok,
                          "ms_call": med(whole), "ms_weights": med(wts), "ms_interp": med(itp), "ms_host_unchecked": med(host),
                          "macs": S * (t + 1) * T, "macs_per_s": round(S * (t + 1) * T / (float(np.median(itp)) * 1e-3), 0),
                          "rounds_ms": {"call": [round(x, 4) for x in whole], "weights": [round(x, 4) for x in wts],
                                        "interp": [round(x, 4) for x in itp], "host": [round(x, 2) for x in host]},
                          "host": socket.gethostname()}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dealing Shamir shares on the device against the multi-dealer encrypt it feeds, interleaved in one process
(run on the GPU box):
    python tools/shamir_timing.py [--steps 20] [--rounds 5]
Three calls, on one stream after pvw_prepare(PVW_PREPARE_MFMA):
  encrypt  pvw_encrypt_multi_device on ready-made shares (the baseline: what a host-side sharing feeds)
  deal     pvw_deal_shares_device (shares made on the device, then the same encrypt)
  shares   pvw_shamir_shares_device alone
at config 3 (n = 4096, k = 256, l = 8, 17 limbs) x 64 dealers for degree 255, 2047 and 4095, and at ref128x (n = 4096, k = 1024,
l = 8, 4 x 56-bit) x 64 dealers for degree 2047, p = 2^61 - 1.  Per round each call runs --steps times back to back between two
HIP events; the order rotates from round to round.  One JSON line per case: median ms per call over the rounds."""
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
from pvw_rs_amd import workloads  # noqa: E402

dev = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
P61 = (1 << 61) - 1


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
    steps, rounds = int(arg("--steps", 20)), int(arg("--rounds", 5))
    D = 64
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for config, degrees in (("c3", (255, 2047, 4095)), ("ref128x", (2047,))):
        n, k, l, L = (4096, 256, 8, 17) if config == "c3" else workloads.ENCRYPT_CONFIGS["ref128x"][:4]
        moduli = workloads.config_moduli(config, L)
        p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()
        gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
        gpk.fill_uniform(SEED)
        lib = p._lib
        s = torch.cuda.Stream(device=dev)
        sp = C.c_void_p(s.cuda_stream)
        p.prepare(P.PREPARE_MFMA, s.cuda_stream)
        rng = np.random.default_rng(1)
        secrets = torch.from_numpy(rng.integers(0, P61, size=D, dtype=np.uint64).view(np.int64)).to(dev)
        sh = torch.from_numpy(rng.integers(0, P61, size=(D, n), dtype=np.uint64).view(np.int64)).to(dev)
        out = torch.empty((D, n), dtype=torch.int64, device=dev)
        c1 = torch.empty((D, k, L, l), dtype=torch.int64, device=dev)
        c2 = torch.empty((D, n, L, l), dtype=torch.int64, device=dev)
        seeds = np.frombuffer(SEED * D, dtype=np.uint8).copy()
        sdp = seeds.ctypes.data_as(C.c_void_p)
        for t in degrees:
            calls = {
                "encrypt": lambda: P.api._check(lib.pvw_encrypt_multi_device(p._h, ptr(sh), D, n, sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp), lib),
                "deal": lambda: P.api._check(lib.pvw_deal_shares_device(p._h, ptr(secrets), D, t, P61, sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp), lib),
                "shares": lambda: P.api._check(lib.pvw_shamir_shares_device(p._h, ptr(secrets), D, t, P61, sdp, None, ptr(out), sp), lib),
            }
            names = list(calls)
            for name in names:                      # warm-up
                timed(calls[name], 3, s)
            acc = {name: [] for name in names}
            for r in range(rounds):
                for name in names[r % 3:] + names[:r % 3]:
                    acc[name].append(timed(calls[name], steps, s))
            med = {name: float(np.median(v)) for name, v in acc.items()}
            print(json.dumps({"config": config, "n": n, "k": k, "l": l, "L": L, "dealers": D, "degree": t, "steps": steps, "rounds": rounds,
                              "ms_encrypt": round(med["encrypt"], 4), "ms_deal": round(med["deal"], 4), "ms_shares": round(med["shares"], 4),
                              "deal_minus_encrypt_ms": round(med["deal"] - med["encrypt"], 4),
                              "terms_per_s": round(D * n * t / (med["shares"] * 1e-3), 0),
                              "rounds_ms": {name: [round(x, 4) for x in v] for name, v in acc.items()},
                              "host": socket.gethostname()}), flush=True)
        del p, gpk


if __name__ == "__main__":
    main()

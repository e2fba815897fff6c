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
HIP events; the order rotates from round to round.  One JSON line per case: median ms per call over the rounds.
    python tools/shamir_timing.py --packed [--secrets 4096] [--steps 3] [--rounds 3]
Packed dealing at config 3: the same S secrets dealt by pvw_deal_shares_packed_device at pack 1, 16 and 64
(D = S / pack dealers, degree n / 2 - pack) beside pvw_deal_shares_device (D = S, degree n / 2 - 1), the share calls alone
(pvw_shamir_shares_device, pvw_shamir_shares_packed_device), and from a profiled pass the part of each packed deal spent in
shamir_eval_kernel<true> and in the weights kernels.  One JSON line."""
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


def packed():
    steps, rounds, S = int(arg("--steps", 3)), int(arg("--rounds", 3)), int(arg("--secrets", 4096))
    n, k, l, L = 4096, 256, 8, 17
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(workloads.config_moduli("c3", L)).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    p.prepare(P.PREPARE_MFMA, s.cuda_stream)
    rng = np.random.default_rng(1)
    secrets = torch.from_numpy(rng.integers(0, P61, size=S, dtype=np.uint64).view(np.int64)).to(dev)
    out = torch.empty((S, n), dtype=torch.int64, device=dev)
    c1 = torch.empty((S, k, L, l), dtype=torch.int64, device=dev)
    c2 = torch.empty((S, n, L, l), dtype=torch.int64, device=dev)
    seeds = np.frombuffer(SEED * S, dtype=np.uint8).copy()
    sdp = seeds.ctypes.data_as(C.c_void_p)
    ok = lambda rc: P.api._check(rc, lib)  # noqa: E731
    calls = {"deal_unpacked": lambda: ok(lib.pvw_deal_shares_device(p._h, ptr(secrets), S, n // 2 - 1, P61, sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp)),
             "shares_unpacked": lambda: ok(lib.pvw_shamir_shares_device(p._h, ptr(secrets), S, n // 2 - 1, P61, sdp, None, ptr(out), sp))}
    packs = [K for K in (1, 16, 64) if S % K == 0]
    for K in packs:
        calls[f"deal_pack{K}"] = lambda K=K: ok(lib.pvw_deal_shares_packed_device(p._h, ptr(secrets), S // K, K, n // 2 - K, P61, sdp, ptr(c1),
                                                                               ptr(c2), P.REPR_NTT, sp))
        calls[f"shares_pack{K}"] = lambda K=K: ok(lib.pvw_shamir_shares_packed_device(p._h, ptr(secrets), S // K, K, n // 2 - K, P61, sdp, None,
                                                                                   ptr(out), sp))
    names = list(calls)
    for name in names:                              # warm-up (sizes the weights of every pack)
        timed(calls[name], 1, s)
    acc = {name: [] for name in names}
    for r in range(rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            acc[name].append(timed(calls[name], steps, s))
    med = {name: round(float(np.median(v)), 4) for name, v in acc.items()}
    # the kernels' part of each packed deal: one profiled call each (every launch bracketed by events, so not a timing of the call)
    part = {}
    p.set_profiling(True)
    for K in packs:
        p.reset_profiling()
        calls[f"deal_pack{K}"]()
        torch.cuda.synchronize()
        ev, wt = p.kernel_time("shamir_eval_packed")[0], p.kernel_time("shamir_packed_weights")[0]
        part[f"pack{K}"] = {"ms_eval_packed": round(ev, 4), "ms_weights": round(wt, 4),
                            "eval_share_of_deal": round(ev / med[f"deal_pack{K}"], 4), "weights_share_of_deal": round(wt / med[f"deal_pack{K}"], 5)}
    p.set_profiling(False)
    print(json.dumps({"config": "c3", "n": n, "k": k, "l": l, "L": L, "secrets": S, "steps": steps, "rounds": rounds, "ms": med,
                      "us_per_secret": {name: round(1e3 * v / S, 3) for name, v in med.items()}, "kernels": part,
                      "rounds_ms": {name: [round(x, 4) for x in v] for name, v in acc.items()}}), flush=True)


if __name__ == "__main__":
    packed() if "--packed" in sys.argv else main()

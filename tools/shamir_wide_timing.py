#!/usr/bin/env python3
"""Dealing Shamir shares over a 256-bit prime field on the device against the multi-dealer encrypt it feeds,
interleaved in one process (run on the GPU box):
    python tools/shamir_wide_timing.py [--steps 5] [--rounds 5]
Three calls, on one stream after pvw_prepare(PVW_PREPARE_MFMA):
  encrypt  pvw_encrypt_multi_device on ready-made limb planes of the same size (D * NL vectors: what a host-side sharing feeds)
  deal     pvw_deal_shares_wide_device (shares made and cut into limbs on the device, then the same encrypt)
  shares   pvw_shamir_shares_wide_device alone
at config 3 (n = 4096, k = 256, l = 8, 17 limbs) x 64 dealers, degree 2047, p = the secp256k1 group order, 52-bit limbs (NL = 5,
320 vectors).  Per round each call runs --steps times back to back between two HIP events; the order rotates from round to
round.  One JSON line: median ms per call over the rounds.
    python tools/shamir_wide_timing.py --packed [--secrets 320] [--steps 3] [--rounds 5]
Packed dealing at config 3: the same S wide secrets dealt by pvw_deal_shares_packed_wide_device at pack 1, 16 and
64 (D = S / pack dealers, degree 2047 - (pack - 1)) beside pvw_deal_shares_wide_device (D = S, degree 2047), the share calls alone
(pvw_shamir_shares_wide_device, pvw_shamir_shares_packed_wide_device), and from a profiled pass the part of each packed deal
spent in shamir_eval_packed_wide_kernel and in the weights kernels.  One JSON line: median and range over the rounds."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: E402

import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import api, workloads  # noqa: E402

dev = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


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


def packed_main():
    S, steps, rounds = int(arg("--secrets", 320)), int(arg("--steps", 3)), int(arg("--rounds", 5))
    limb_bits, pm, packs = 52, SECP_N, (1, 16, 64)
    n, k, l, L = 4096, 256, 8, 17
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(workloads.config_moduli("c3", L)).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    p.prepare(P.PREPARE_MFMA, s.cuda_stream)
    NL = P.shamir_wide_limbs(pm, limb_bits)
    rng = np.random.default_rng(1)
    secrets = torch.from_numpy(rng.integers(0, 1 << 62, size=(S, 4), dtype=np.uint64).view(np.int64)).to(dev)
    out = torch.empty((S, n, 4), dtype=torch.int64, device=dev)
    c1 = torch.empty((S * NL, k, L, l), dtype=torch.int64, device=dev)
    c2 = torch.empty((S * NL, n, L, l), dtype=torch.int64, device=dev)
    seeds = np.frombuffer(SEED * (S * NL), dtype=np.uint8).copy()
    sdp = seeds.ctypes.data_as(C.c_void_p)
    pmp = api._wide_modulus(pm).ctypes.data_as(C.c_void_p)
    ok = lambda rc: api._check(rc, lib)  # noqa: E731
    t0 = n // 2 - 1
    calls = {
        "deal_wide": lambda: ok(lib.pvw_deal_shares_wide_device(p._h, ptr(secrets), S, t0, pmp, limb_bits, sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp)),
        "shares_wide": lambda: ok(lib.pvw_shamir_shares_wide_device(p._h, ptr(secrets), S, t0, pmp, sdp, None, ptr(out), sp)),
    }
    for K in packs:
        calls[f"deal_pack{K}"] = lambda K=K: ok(lib.pvw_deal_shares_packed_wide_device(p._h, ptr(secrets), S // K, K, t0 - (K - 1), pmp, limb_bits,
                                                                                        sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp))
        calls[f"shares_pack{K}"] = lambda K=K: ok(lib.pvw_shamir_shares_packed_wide_device(p._h, ptr(secrets), S // K, K, t0 - (K - 1), pmp, sdp,
                                                                                            None, ptr(out), sp))
    names = list(calls)
    for name in names:                      # warm-up; the largest pack sizes the weights
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
        ev, wt = p.kernel_time("shamir_eval_packed_wide")[0], p.kernel_time("shamir_packed_wide_weights")[0]
        part[f"pack{K}"] = {"ms_eval_packed": round(ev, 4), "ms_weights": round(wt, 4),
                            "eval_share_of_deal": round(ev / med[f"deal_pack{K}"], 4), "weights_share_of_deal": round(wt / med[f"deal_pack{K}"], 5)}
    p.set_profiling(False)
    print(json.dumps({"config": "c3", "n": n, "k": k, "l": l, "L": L, "secrets": S, "plain_modulus_bits": pm.bit_length(), "limb_bits": limb_bits,
                      "num_limbs": NL, "steps": steps, "rounds": rounds, "ms": med,
                      "range_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in acc.items()},
                      "us_per_secret": {name: round(1e3 * v / S, 3) for name, v in med.items()}, "kernels": part,
                      "rounds_ms": {name: [round(x, 4) for x in v] for name, v in acc.items()}}), flush=True)


def main():
    if "--packed" in sys.argv:
        return packed_main()
    steps, rounds = int(arg("--steps", 5)), int(arg("--rounds", 5))
    D, t, limb_bits, pm = 64, 2047, 52, SECP_N
    n, k, l, L = 4096, 256, 8, 17
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(workloads.config_moduli("c3", L)).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    p.prepare(P.PREPARE_MFMA, s.cuda_stream)
    NL = P.shamir_wide_limbs(pm, limb_bits)
    V = D * NL
    rng = np.random.default_rng(1)
    secrets = torch.from_numpy(rng.integers(0, 1 << 62, size=(D, 4), dtype=np.uint64).view(np.int64)).to(dev)
    planes = torch.from_numpy(rng.integers(0, 1 << limb_bits, size=(V, n), dtype=np.uint64).view(np.int64)).to(dev)
    out = torch.empty((D, n, 4), dtype=torch.int64, device=dev)
    c1 = torch.empty((V, k, L, l), dtype=torch.int64, device=dev)
    c2 = torch.empty((V, n, L, l), dtype=torch.int64, device=dev)
    seeds = np.frombuffer(SEED * V, dtype=np.uint8).copy()
    sdp = seeds.ctypes.data_as(C.c_void_p)
    pmw = api._wide_modulus(pm)
    pmp = pmw.ctypes.data_as(C.c_void_p)
    ok = lambda rc: api._check(rc, lib)  # noqa: E731
    calls = {
        "encrypt": lambda: ok(lib.pvw_encrypt_multi_device(p._h, ptr(planes), V, n, sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp)),
        "deal": lambda: ok(lib.pvw_deal_shares_wide_device(p._h, ptr(secrets), D, t, pmp, limb_bits, sdp, ptr(c1), ptr(c2), P.REPR_NTT, sp)),
        "shares": lambda: ok(lib.pvw_shamir_shares_wide_device(p._h, ptr(secrets), D, t, pmp, sdp, None, ptr(out), sp)),
    }
    names = list(calls)
    for name in names:                      # warm-up
        timed(calls[name], 2, s)
    acc = {name: [] for name in names}
    for r in range(rounds):
        for name in names[r % 3:] + names[:r % 3]:
            acc[name].append(timed(calls[name], steps, s))
    med = {name: float(np.median(v)) for name, v in acc.items()}
    print(json.dumps({"config": "c3", "n": n, "k": k, "l": l, "L": L, "dealers": D, "degree": t, "plain_modulus_bits": pm.bit_length(),
                      "limb_bits": limb_bits, "num_limbs": NL, "vectors": V, "steps": steps, "rounds": rounds,
                      "ms_encrypt": round(med["encrypt"], 4), "ms_deal": round(med["deal"], 4), "ms_shares": round(med["shares"], 4),
                      "deal_minus_encrypt_ms": round(med["deal"] - med["encrypt"], 4),
                      "terms_per_s": round(D * n * t / (med["shares"] * 1e-3), 0),
                      "rounds_ms": {name: [round(x, 4) for x in v] for name, v in acc.items()}}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Share repair on the device beside the corrected call it extends, in one process (run on the GPU box):
    python tools/evaluate_timing.py [--steps 3] [--rounds 5]
pvw_shamir_evaluate_corrected_device on one stream, on shares made by pvw_shamir_shares_device, count = 4096, t = 2047 (r = 2048,
E = 1024), p = 2^61 - 1, at S in {64, 1024} and T in {64, 4096} targets, once on the consistent sharing and once with 1024 whole
columns overwritten.  The sharing is dealt among 8192 parties and the first 4096 are the input, so the targets are either
"columns" (the first T indices: a right column is read back, a wrong one divides) or "off" (indices 4096 .. 4096 + T, parties
that were never an input: one Fermat inversion per secret and target); both are checked against the dealt shares.  Every round
times --steps evaluate calls and then --steps corrected calls on the same input, so the two are interleaved:
  evaluate   the whole call between two HIP events, after warm-up
  corrected  pvw_shamir_reconstruct_corrected_device on the same input, as a whole: the yardstick
and, from the context's profiling scopes of the evaluate call:
  weights    the corrected call's public matrices (shamir_correct_weights)
  decode     syndromes, Berlekamp-Massey, locator values, finish (shamir_correct)
  eval_wts   the target groups' public matrices: scale, Cauchy matrix, powers (shamir_evaluate_weights)
  eval       y o M, the three products and the finish pass (shamir_evaluate)
One JSON line per shape and input: median ms over the rounds, and the rounds."""
import ctypes as C
import itertools
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
SCOPES = (("weights", "shamir_correct_weights"), ("decode", "shamir_correct"), ("eval_wts", "shamir_evaluate_weights"),
          ("eval", "shamir_evaluate"))


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
    n, t, Smax, Tmax, N = 4096, 2047, 1024, 4096, 8192
    E = (n - t - 1) // 2
    p = P.PvwParametersBuilder().set_parties(N).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rng = np.random.default_rng(1)
    secrets = rng.integers(0, P61, size=Smax, dtype=np.uint64)
    d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
    seeds = rng.integers(0, 256, size=Smax * 32, dtype=np.uint8)
    clean = torch.empty((Smax, N), dtype=torch.int64, device=dev)
    P.api._check(lib.pvw_shamir_shares_device(p._h, ptr(d_se), Smax, t, P61, seeds.ctypes.data_as(C.c_void_p), None, ptr(clean), sp), lib)
    s.synchronize()
    planted = np.sort(rng.choice(n, size=E, replace=False))
    bent = clean.clone()
    junk = torch.from_numpy(rng.integers(1, P61, size=(Smax, E), dtype=np.int64)).to(dev)
    bent[:, planted] = (bent[:, planted] + junk) % P61
    ix = np.arange(n, dtype=np.uint64)
    ixp = ix.ctypes.data_as(C.c_void_p)
    values = torch.empty((Smax, Tmax), dtype=torch.int64, device=dev)
    out = torch.empty(Smax, dtype=torch.int64, device=dev)
    nerr = torch.empty(Smax, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty((Smax, n // 64), dtype=torch.int64, device=dev)
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    for S, T, (kind, first) in itertools.product((64, Smax), (64, Tmax), (("columns", 0), ("off", n))):
        tg = np.arange(first, first + T, dtype=np.uint64)
        tgp = tg.ctypes.data_as(C.c_void_p)
        vals = values.view(-1)[:S * T].view(S, T)
        for name, shares, want_err in (("consistent", clean, 0), ("at_the_bound", bent, E)):
            call = lambda: P.api._check(lib.pvw_shamir_evaluate_corrected_device(p._h, P61, t, ixp, n, ptr(shares), S, N, 1, tgp, T,  # noqa: E731
                                                                                 ptr(vals), ptr(out), ptr(nerr), ptr(col), ptr(mask), sp), lib)
            old = lambda: P.api._check(lib.pvw_shamir_reconstruct_corrected_device(p._h, P61, t, ixp, n, ptr(shares), S, N, 1, ptr(out),  # noqa: E731
                                                                                   ptr(nerr), ptr(col), ptr(mask), sp), lib)
            timed(call, 1, s)                                       # warm-up (sizes the workspace)
            ok = (bool((out[:S].cpu().numpy().view(np.uint64) == secrets[:S]).all()) and bool((nerr[:S] == want_err).all().item())
                  and bool(torch.equal(vals, clean[:S, first:first + T])))
            timed(old, 1, s)
            whole, base = [], []
            for _ in range(rounds):
                whole.append(timed(call, steps, s))
                base.append(timed(old, steps, s))
            scopes = {k: [] for k, _ in SCOPES}
            p.set_profiling(True)
            for _ in range(rounds):
                p.reset_profiling()
                timed(call, steps, s)
                for k, scope in SCOPES:
                    scopes[k].append(p.kernel_time(scope)[0] / steps)
            p.set_profiling(False)
            rec = {"S": S, "T": T, "targets": kind, "count": n, "degree": t, "input": name, "steps": steps, "rounds": rounds, "correct": ok,
                   "ms_evaluate": med(whole), "ms_corrected": med(base), "ms_difference": round(med(whole) - med(base), 4)}
            rec.update({"ms_" + k: med(v) for k, v in scopes.items()})
            rec["rounds_ms"] = {"evaluate": [round(x, 4) for x in whole], "corrected": [round(x, 4) for x in base],
                                **{k: [round(x, 4) for x in v] for k, v in scopes.items()}}
            rec["host"] = socket.gethostname()
            print(json.dumps(rec), flush=True)

if __name__ == "__main__":
    main()

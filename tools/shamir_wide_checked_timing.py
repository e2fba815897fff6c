#!/usr/bin/env python3
"""Checked Shamir reconstruction over a 256-bit prime field on the device, in one process (run on the GPU box):
    python tools/shamir_wide_checked_timing.py [--steps 3] [--rounds 7]
pvw_shamir_reconstruct_wide_checked_device on one stream, on shares made by pvw_shamir_shares_wide_device (a consistent sharing:
nothing deviates, so no atomic is issued), at S = 64 secrets, count = 4096, t = 2047 over the order of secp256k1:
  call      the whole call between two HIP events, --steps calls back to back, after warm-up
  weights   the points, shamir_prod_wide_kernel and shamir_weights_wide_kernel, from the context's profiling scopes
  interp    shamir_interp_wide_kernel (with the kernel that clears bad), likewise; profiling is switched on for rounds of its own
and pvw_shamir_wide_from_limbs_device on 4096 x 64 elements of NL = 5 limbs of 52 bits, side by side (strides (1, NL)), between
two HIP events.  One JSON line per measurement: median, minimum and maximum ms over the rounds, and the rounds themselves."""
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
from pvw_rs_amd import api  # noqa: E402

dev = torch.device("cuda", 0)
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
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


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4),
            "rounds_ms": [round(float(x), 4) for x in v]}


def main():
    steps, rounds = int(arg("--steps", 3)), int(arg("--rounds", 7))
    n, t, S, lb, nl = 4096, 2047, 64, 52, 5
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    nptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(1)
    pm = api._wide_modulus(SECP_N)
    secrets = rng.integers(0, 1 << 63, size=(S, 4), dtype=np.uint64)
    d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
    seeds = rng.integers(0, 256, size=S * 32, dtype=np.uint8)
    shares = torch.empty((S, n, 4), dtype=torch.int64, device=dev)
    api._check(lib.pvw_shamir_shares_wide_device(p._h, ptr(d_se), S, t, nptr(pm), nptr(seeds), None, ptr(shares), sp), lib)
    s.synchronize()
    ix = np.arange(n, dtype=np.uint64)
    out = torch.empty((S, 4), dtype=torch.int64, device=dev)
    bad = torch.empty(S, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    call = lambda: api._check(lib.pvw_shamir_reconstruct_wide_checked_device(p._h, nptr(pm), t, nptr(ix), n, ptr(shares), S, n, 1,  # noqa: E731
                                                                             ptr(out), ptr(bad), ptr(col), sp), lib)
    timed(call, 2, s)                                           # warm-up (sizes the workspace)
    ok = api._wide_ints(out.cpu().numpy().view(np.uint64)) == api._wide_ints(secrets) and not bad.any().item() and not col.any().item()
    whole = [timed(call, steps, s) for _ in range(rounds)]
    wts, itp = [], []
    p.set_profiling(True)
    for _ in range(rounds):
        p.reset_profiling()
        timed(call, steps, s)
        wts.append(p.kernel_time("shamir_weights_wide")[0] / steps)
        itp.append(p.kernel_time("shamir_interp_wide")[0] / steps)
    p.set_profiling(False)
    T = n - t
    base = {"host": socket.gethostname(), "steps": steps, "rounds": rounds}
    print(json.dumps(dict(base, what="reconstruct_wide_checked", S=S, count=n, degree=t, correct=bool(ok), weights_bytes=(t + 1) * T * 32,
                          products=S * (t + 1) * T, ms_call=stats(whole), ms_weights=stats(wts), ms_interp=stats(itp))), flush=True)
    # the fold: [4096][64 * 5] words as a decrypt-all leaves them, any words
    limbs = torch.from_numpy(rng.integers(0, 1 << 63, size=(n, S * nl), dtype=np.int64)).to(dev)
    folded = torch.empty((n * S, 4), dtype=torch.int64, device=dev)
    fold = lambda: api._check(lib.pvw_shamir_wide_from_limbs_device(p._h, nptr(pm), ptr(limbs), n * S, 1, nl, lb, nl, ptr(folded), sp), lib)  # noqa: E731
    timed(fold, 2, s)
    sample = limbs[:2].cpu().numpy().view(np.uint64).reshape(2 * S, nl)
    want = api._wide(P.shamir_wide_from_limbs(sample.T.tolist(), SECP_N, lb))
    ok = bool(np.array_equal(folded[:2 * S].cpu().numpy().view(np.uint64), want))
    fl = [timed(fold, steps, s) for _ in range(rounds)]
    print(json.dumps(dict(base, what="wide_from_limbs_device", elements=n * S, num_limbs=nl, limb_bits=lb, correct=ok, ms_fold=stats(fl))),
          flush=True)


if __name__ == "__main__":
    main()

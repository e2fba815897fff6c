#!/usr/bin/env python3
"""Corrected Shamir reconstruction over a 256-bit prime field on the device, in one process (run on the GPU box):
    python tools/shamir_wide_corrected_timing.py [--steps 3] [--rounds 7]
pvw_shamir_reconstruct_wide_corrected_device on one stream, on shares made by pvw_shamir_shares_wide_device, at S = 64 secrets,
count = 4096, t = 2047 (r = 2048, E = 1024) over the order of secp256k1 -- once on the consistent sharing (every discrepancy is
0: the locator stays 1) and once with 1024 columns overwritten by random words in every row (E errors: the locator grows to its
full degree and the finish pass issues 64 x 1024 atomics):
  call      the whole call between two HIP events, --steps calls back to back, after warm-up
  public    the points, shamir_prod_wide_kernel, the lambda, V and X kernels, from the context's profiling scopes
  decode    the two products, shamir_bm_wide_kernel and the finish pass, likewise; profiling is switched on for rounds of its own
and pvw_shamir_reconstruct_wide_checked_device on the same input in the same run, as context (its basis is columns 0..t, so on
the overwritten input it reports and does not recover).  One JSON line per measurement: median, minimum and maximum ms over the
rounds, and the rounds themselves."""
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
    n, t, S, nbad = 4096, 2047, 64, 1024
    E = (n - t - 1) // 2
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
    clean = torch.empty((S, n, 4), dtype=torch.int64, device=dev)
    api._check(lib.pvw_shamir_shares_wide_device(p._h, ptr(d_se), S, t, nptr(pm), nptr(seeds), None, ptr(clean), sp), lib)
    s.synchronize()
    cols = np.sort(rng.choice(n, size=nbad, replace=False))
    spoiled = clean.clone()
    spoiled[:, torch.from_numpy(cols).to(dev)] = torch.from_numpy(rng.integers(0, 1 << 63, size=(S, nbad, 4), dtype=np.int64)).to(dev)
    ix = np.arange(n, dtype=np.uint64)
    W = (n + 63) // 64
    out = torch.empty((S, 4), dtype=torch.int64, device=dev)
    nerr = torch.empty(S, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty((S, W), dtype=torch.int64, device=dev)
    bad = torch.empty(S, dtype=torch.int32, device=dev)
    base = {"host": socket.gethostname(), "steps": steps, "rounds": rounds, "S": S, "count": n, "degree": t, "E": E}
    for name, shares, want_nerr in (("consistent", clean, 0), (f"{nbad}_columns_overwritten", spoiled, nbad)):
        call = lambda: api._check(lib.pvw_shamir_reconstruct_wide_corrected_device(  # noqa: E731
            p._h, nptr(pm), t, nptr(ix), n, ptr(shares), S, n, 1, ptr(out), ptr(nerr), ptr(col), ptr(mask), sp), lib)
        timed(call, 2, s)                                       # warm-up (sizes the workspace)
        want_col = np.zeros(n, dtype=np.int32)
        want_col[cols] = S if want_nerr else 0
        ok = (api._wide_ints(out.cpu().numpy().view(np.uint64)) == api._wide_ints(secrets) and (nerr == want_nerr).all().item()
              and np.array_equal(col.cpu().numpy(), want_col))
        whole = [timed(call, steps, s) for _ in range(rounds)]
        pub, dec = [], []
        p.set_profiling(True)
        for _ in range(rounds):
            p.reset_profiling()
            timed(call, steps, s)
            pub.append(p.kernel_time("shamir_correct_wide_weights")[0] / steps)
            dec.append(p.kernel_time("shamir_correct_wide")[0] / steps)
        p.set_profiling(False)
        print(json.dumps(dict(base, what="reconstruct_wide_corrected", input=name, correct=bool(ok), ms_call=stats(whole),
                              ms_public=stats(pub), ms_decode=stats(dec))), flush=True)
        chk = lambda: api._check(lib.pvw_shamir_reconstruct_wide_checked_device(p._h, nptr(pm), t, nptr(ix), n, ptr(shares), S, n, 1,  # noqa: E731
                                                                                ptr(out), ptr(bad), ptr(col), sp), lib)
        timed(chk, 2, s)
        recovered = api._wide_ints(out.cpu().numpy().view(np.uint64)) == api._wide_ints(secrets)
        whole = [timed(chk, steps, s) for _ in range(rounds)]
        print(json.dumps(dict(base, what="reconstruct_wide_checked", input=name, recovered=bool(recovered), ms_call=stats(whole))), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Shamir reconstruction with erasures over a 256-bit prime field on the device, in one process (run on the GPU box):
    python tools/shamir_wide_erasures_timing.py [--steps 3] [--rounds 7]
pvw_shamir_reconstruct_wide_erasures_device on one stream, on shares made by pvw_shamir_shares_wide_device, at S = 64 secrets,
count = 4096, t = 2047 (r = 2048) over the order of secp256k1, each case interleaved round by round with
pvw_shamir_reconstruct_wide_corrected_device on the same input:
  no_mask                       erased = NULL on the consistent sharing: the wide corrected call behind the argument checks
  1024_erased                   1024 columns overwritten by random words in every row and flagged, against the same columns unflagged
                                (the corrected call finds them as E = 1024 errors)
  2048_erased                   2048 columns overwritten and flagged: r erasures, no error; the corrected call gives up
  1024_erased_512_overwritten   1024 flagged and 512 more overwritten: 2 * 512 + 1024 = r; the corrected call gives up
Every run is checked against the dealt secrets and the expected nerr.  Times are whole calls between two HIP events, --steps calls
back to back, after warm-up; the calls are not split by kernel.  One JSON line per case: median, minimum and maximum ms over the
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
UNDECODABLE = 0xFFFFFFFF


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
    n, t, S = 4096, 2047, 64
    r = n - t - 1
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    nptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(1)
    pm = api._wide_modulus(SECP_N)
    secrets = rng.integers(0, 1 << 63, size=(S, 4), dtype=np.uint64)
    d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
    seeds = rng.integers(0, 256, size=S * 32, dtype=np.uint8)
    clean = torch.empty((S, n, 4), dtype=torch.int64, device=dev)
    api._check(lib.pvw_shamir_shares_wide_device(p._h, ptr(d_se), S, t, nptr(pm), nptr(seeds), None, ptr(clean), sp), lib)
    s.synchronize()
    order = rng.permutation(n)
    ix = np.arange(n, dtype=np.uint64)
    W = (n + 63) // 64
    out = torch.empty((S, 4), dtype=torch.int64, device=dev)
    nerr = torch.empty(S, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty((S, W), dtype=torch.int64, device=dev)

    def inputs(n_erased, n_over):
        """the shares with n_erased + n_over columns overwritten by random words in every row, and the mask of the first n_erased"""
        cols = order[:n_erased + n_over]
        shares = clean.clone()
        if len(cols):
            junk = rng.integers(0, 1 << 63, size=(S, len(cols), 4), dtype=np.int64)
            shares[:, torch.from_numpy(np.sort(cols)).to(dev)] = torch.from_numpy(junk).to(dev)
        er = np.zeros((S, W), dtype=np.uint64)
        for c in order[:n_erased]:
            er[:, c // 64] |= np.uint64(1 << (int(c) % 64))
        return shares, torch.from_numpy(er.view(np.int64)).to(dev)

    def report(want_nerr):
        got = nerr.cpu().numpy().view(np.uint32)
        secrets_ok = api._wide_ints(out.cpu().numpy().view(np.uint64)) == api._wide_ints(secrets)
        if want_nerr == UNDECODABLE:
            return bool((got == UNDECODABLE).all() and not out.any().item())
        return bool(secrets_ok and (got == want_nerr).all())

    base = {"host": socket.gethostname(), "steps": steps, "rounds": rounds, "S": S, "count": n, "degree": t, "r": r}
    E = r // 2
    for name, n_erased, n_over, masked in (("no_mask", 0, 0, False), ("1024_erased", 1024, 0, True), ("2048_erased", 2048, 0, True),
                                           ("1024_erased_512_overwritten", 1024, 512, True)):
        shares, d_er = inputs(n_erased, n_over)
        new = lambda: api._check(lib.pvw_shamir_reconstruct_wide_erasures_device(  # noqa: E731
            p._h, nptr(pm), t, nptr(ix), n, ptr(shares), S, n, 1, ptr(d_er) if masked else None, ptr(out), ptr(nerr), ptr(col), ptr(mask),
            sp), lib)
        old = lambda: api._check(lib.pvw_shamir_reconstruct_wide_corrected_device(  # noqa: E731
            p._h, nptr(pm), t, nptr(ix), n, ptr(shares), S, n, 1, ptr(out), ptr(nerr), ptr(col), ptr(mask), sp), lib)
        bad = n_erased + n_over
        timed(new, 2, s)                                        # warm-up (sizes the workspace)
        ok_new = report(n_over)
        timed(old, 2, s)
        ok_old = report(bad if bad <= E else UNDECODABLE)
        t_new, t_old = [], []
        for _ in range(rounds):                                 # interleaved round by round
            t_new.append(timed(new, steps, s))
            t_old.append(timed(old, steps, s))
        timed(new, 1, s)
        ok_new = ok_new and report(n_over)
        print(json.dumps(dict(base, what="reconstruct_wide_erasures", input=name, erased=n_erased, overwritten=n_over, correct=ok_new,
                              corrected_call_as_expected=ok_old, corrected_call_nerr=(bad if bad <= E else "undecodable"),
                              ms_erasures_call=stats(t_new), ms_corrected_call=stats(t_old))), flush=True)
        if not (ok_new and ok_old):
            sys.exit(1)


if __name__ == "__main__":
    main()

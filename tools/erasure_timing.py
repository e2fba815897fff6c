#!/usr/bin/env python3
"""Shamir reconstruction with erasures on the device beside the corrected call it extends, in one process (run on
the GPU box):
    python tools/erasure_timing.py [--steps 3] [--rounds 5]
count = 4096, t = 2047 (r = 2048), p = 2^61 - 1, shares made by pvw_shamir_shares_device, at S = 64 and S = 1024.  Per case the
erasure call and, where it can decode the input, pvw_shamir_reconstruct_corrected_device, interleaved round by round, each
--steps calls back to back between two HIP events after a warm-up call that sizes the workspace:
  no_mask        erased = NULL on the consistent sharing                     beside the corrected call on the same input
  erased_1024    1024 whole columns erased and filled with junk              beside the corrected call with the same 1024 overwritten
  erased_2048    2048 columns erased: r of them                              the corrected call cannot decode this
  erased_1024_wrong_512   1024 erased plus 512 overwritten                   the corrected call cannot decode this
  evaluate_64    the evaluate form of erased_1024_wrong_512 at T = 64 targets
with the erasure call's two scopes (weights: the public matrices, X at r + 1 rows; decode: syndromes, Gamma, Forney syndromes,
Berlekamp-Massey, Psi, locator values, finish) from the context's profiling.  One JSON line per shape and case: median ms over
the rounds, and the rounds."""
import ctypes as C
import json
import os
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


def mask_rows(cols, n, S):
    m = np.zeros(n // 64, dtype=np.uint64)
    for c in cols:
        m[c // 64] |= np.uint64(1 << (c % 64))
    return torch.from_numpy(np.tile(m, (S, 1)).view(np.int64)).to(dev)


def main():
    steps, rounds = int(arg("--steps", 3)), int(arg("--rounds", 5))
    n, t, Smax, T = 4096, 2047, 1024, 64
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    rng = np.random.default_rng(1)
    secrets = rng.integers(0, P61, size=Smax, dtype=np.uint64)
    d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
    seeds = rng.integers(0, 256, size=Smax * 32, dtype=np.uint8)
    clean = torch.empty((Smax, n), dtype=torch.int64, device=dev)
    P.api._check(lib.pvw_shamir_shares_device(p._h, ptr(d_se), Smax, t, P61, seeds.ctypes.data_as(C.c_void_p), None, ptr(clean), sp), lib)
    s.synchronize()
    order = rng.permutation(n)
    junk = torch.from_numpy(rng.integers(1, P61, size=(Smax, 2048), dtype=np.int64)).to(dev)

    def overwritten(cols):
        x = clean.clone()
        x[:, cols] = (x[:, cols] + junk[:, :len(cols)]) % P61
        return x

    e1024, e2048, w512 = order[:1024], order[:2048], order[1024:1536]
    inputs = {
        "no_mask": (clean, None, clean, 0, 0),
        "erased_1024": (overwritten(e1024), e1024, overwritten(e1024), 0, 1024),
        "erased_2048": (overwritten(e2048), e2048, None, 0, None),
        "erased_1024_wrong_512": (overwritten(order[:1536]), e1024, None, 512, None),
    }
    ix = np.arange(n, dtype=np.uint64)
    ixp = ix.ctypes.data_as(C.c_void_p)
    tg = np.concatenate([e1024[:32], w512[:16], np.arange(n, n + 16)]).astype(np.uint64)
    tgp = tg.ctypes.data_as(C.c_void_p)
    out = torch.empty(Smax, dtype=torch.int64, device=dev)
    nerr = torch.empty(Smax, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty((Smax, n // 64), dtype=torch.int64, device=dev)
    values = torch.empty((Smax, T), dtype=torch.int64, device=dev)
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
    for S in (64, Smax):
        cases = [(name, False) + v for name, v in inputs.items()] + [("evaluate_64", True) + inputs["erased_1024_wrong_512"]]
        for name, evaluate, shares, cols, old_shares, want_new, want_old in cases:
            er = None if cols is None else mask_rows(cols, n, S)
            if evaluate:
                new = lambda: P.api._check(lib.pvw_shamir_evaluate_erasures_device(p._h, P61, t, ixp, n, ptr(shares), S, n, 1, ptr(er), tgp, T,  # noqa: E731
                                                                                   ptr(values), ptr(out), ptr(nerr), ptr(col), ptr(mask), sp), lib)
            else:
                new = lambda: P.api._check(lib.pvw_shamir_reconstruct_erasures_device(p._h, P61, t, ixp, n, ptr(shares), S, n, 1, ptr(er),  # noqa: E731
                                                                                      ptr(out), ptr(nerr), ptr(col), ptr(mask), sp), lib)
            old = None
            if old_shares is not None:
                old = lambda: P.api._check(lib.pvw_shamir_reconstruct_corrected_device(p._h, P61, t, ixp, n, ptr(old_shares), S, n, 1, ptr(out),  # noqa: E731
                                                                                       ptr(nerr), ptr(col), ptr(mask), sp), lib)
                timed(old, 1, s)
                ok_old = bool((out[:S].cpu().numpy().view(np.uint64) == secrets[:S]).all()) and bool((nerr[:S] == want_old).all().item())
            timed(new, 1, s)
            ok = bool((out[:S].cpu().numpy().view(np.uint64) == secrets[:S]).all()) and bool((nerr[:S] == want_new).all().item())
            if evaluate:
                ok = ok and bool(torch.equal(values[:S, :48], clean[:S][:, tg[:48].astype(np.int64)]))   # the erased and wrong columns
            t_new, t_old = [], []
            for _ in range(rounds):                                  # the sides interleaved
                t_new.append(timed(new, steps, s))
                if old:
                    t_old.append(timed(old, steps, s))
            wts, dec = [], []
            p.set_profiling(True)
            for _ in range(rounds):
                p.reset_profiling()
                timed(new, steps, s)
                wts.append(p.kernel_time("shamir_correct_weights")[0] / steps)
                dec.append(p.kernel_time("shamir_correct")[0] / steps)
            p.set_profiling(False)
            row = {"S": S, "count": n, "degree": t, "case": name, "steps": steps, "rounds": rounds, "correct": ok, "ms_erasures": med(t_new),
                   "ms_weights": med(wts), "ms_decode": med(dec),
                   "rounds_ms": {"erasures": rnd(t_new), "weights": rnd(wts), "decode": rnd(dec)}}
            if old:
                row.update(ms_corrected=med(t_old), corrected_correct=ok_old)
                row["rounds_ms"]["corrected"] = rnd(t_old)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

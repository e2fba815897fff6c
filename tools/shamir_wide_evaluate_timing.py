#!/usr/bin/env python3
"""Share repair over a 256-bit prime field on the device, run on the GPU box:
    python tools/shamir_wide_evaluate_timing.py [--steps 2] [--rounds 5] [--limit 240] [--case T:targets:input]
pvw_shamir_evaluate_wide_corrected_device / _erasures_device on one stream, on shares made by pvw_shamir_shares_wide_device for
8192 parties of which the first 4096 are the input: S = 64 secrets, count = 4096, t = 2047 (r = 2048) over the order of secp256k1.
  T        64 or 4096 targets
  targets  columns: the first T indices (a right column is read back, a wrong or erased one divides)
           off:     indices 4096 .. 4096 + T, parties that were never an input (one inversion per value)
  input    consistent | 1024_overwritten (no mask; against pvw_shamir_reconstruct_wide_corrected_device)
           1024_erased | 1024_erased_512_overwritten (with a mask; against pvw_shamir_reconstruct_wide_erasures_device)
Each case is interleaved round by round with the decode-only call on the same input; the quantity of interest is the difference.
Every run is checked against the dealt shares at the targets and the dealt secrets.  Times are whole calls between two HIP
events, --steps calls back to back, after warm-up.  Without --case every case runs in a child process of its own under a time
limit of --limit seconds, and the first failure ends the run.  One JSON line per case: median, minimum and maximum ms over the
rounds, the rounds themselves, and the secrets per pass of either call.
    python tools/shamir_wide_evaluate_timing.py --points [--steps 2] [--rounds 5]
The packed secrets in one call against the route the library offered before it, in ONE process: 64 packed rows
(pvw_shamir_shares_packed_wide_device), count = 4096, polynomial degree 2047 (t = 2048 - K), K in {16, 64}; inputs consistent,
1024 columns overwritten, 1024 columns erased.  One side is pvw_shamir_packed_wide_secrets_device; the other is
pvw_shamir_evaluate_wide_corrected_device / _erasures_device at the first t + K columns, the copy of those corrected shares to the
host and pvw_shamir_reconstruct_packed_wide on them, all between the two HIP events.  The sides alternate round by round; both
are checked against the dealt secrets.  One JSON line per case."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
MODULI = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]
INPUTS = {"consistent": (0, 0, False), "1024_overwritten": (0, 1024, False), "1024_erased": (1024, 0, True),
          "1024_erased_512_overwritten": (1024, 512, True)}
CASES = [f"{T}:{tg}:{inp}" for T in (64, 4096) for tg in ("columns", "off") for inp in INPUTS]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4),
            "rounds_ms": [round(float(x), 4) for x in v]}


def passes(S, count, r, nk, Tg=None):
    """secrets per pass by the library's rule (64 MiB of per-secret scratch): the decode-only call, or the evaluation with Tg"""
    per = (count + r + nk) * 32 + 4 if Tg is None else (2 * count + r + nk + 3 * Tg + 1) * 32 + 8
    return min(S, max(1, (64 << 20) // per))


def group(count, nk, T):
    tg = (64 << 20) // ((count + 2 * nk + 2) * 32 + 4)
    if tg > 64:
        tg -= tg % 64
    return min(max(tg, 1), T)


def run_case(case, steps, rounds):
    import torch

    import pvw_rs_amd as P
    from pvw_rs_amd import api

    T, which, inp = case.split(":")
    T = int(T)
    n_erased, n_over, masked = INPUTS[inp]
    dev = torch.device("cuda", 0)
    N, n, t, S = 8192, 4096, 2047, 64
    r = n - t - 1
    p = P.PvwParametersBuilder().set_parties(N).set_dimension(2).set_l(8).set_moduli(MODULI).build()
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
    dealt = torch.empty((S, N, 4), dtype=torch.int64, device=dev)
    api._check(lib.pvw_shamir_shares_wide_device(p._h, ptr(d_se), S, t, nptr(pm), nptr(seeds), None, ptr(dealt), sp), lib)
    s.synchronize()
    order = rng.permutation(n)
    ix = np.arange(n, dtype=np.uint64)
    tg = np.arange(T, dtype=np.uint64) + np.uint64(0 if which == "columns" else n)
    W = (n + 63) // 64
    val = torch.empty((S, T, 4), dtype=torch.int64, device=dev)
    out = torch.empty((S, 4), dtype=torch.int64, device=dev)
    nerr = torch.empty(S, dtype=torch.int32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty((S, W), dtype=torch.int64, device=dev)
    cols = order[:n_erased + n_over]
    shares = dealt[:, :n].clone()
    if len(cols):
        junk = rng.integers(0, 1 << 63, size=(S, len(cols), 4), dtype=np.int64)
        shares[:, torch.from_numpy(np.sort(cols)).to(dev)] = torch.from_numpy(junk).to(dev)
    er = np.zeros((S, W), dtype=np.uint64)
    for c in order[:n_erased]:
        er[:, c // 64] |= np.uint64(1 << (int(c) % 64))
    d_er = torch.from_numpy(er.view(np.int64)).to(dev) if masked else None
    truth = dealt[:, torch.from_numpy(tg.astype(np.int64)).to(dev)]

    def correct(values):
        got = nerr.cpu().numpy().view(np.uint32)
        ok = api._wide_ints(out.cpu().numpy().view(np.uint64)) == api._wide_ints(secrets) and bool((got == n_over).all())
        return ok and (not values or bool(torch.equal(val, truth)))

    head = (p._h, nptr(pm), t, nptr(ix), n, ptr(shares), S, n, 1)
    tail = (ptr(out), ptr(nerr), ptr(col), ptr(mask), sp)
    if masked:
        new = lambda: api._check(lib.pvw_shamir_evaluate_wide_erasures_device(*head, ptr(d_er), nptr(tg), T, ptr(val), *tail), lib)  # noqa: E731
        old = lambda: api._check(lib.pvw_shamir_reconstruct_wide_erasures_device(*head, ptr(d_er), *tail), lib)  # noqa: E731
    else:
        new = lambda: api._check(lib.pvw_shamir_evaluate_wide_corrected_device(*head, nptr(tg), T, ptr(val), *tail), lib)  # noqa: E731
        old = lambda: api._check(lib.pvw_shamir_reconstruct_wide_corrected_device(*head, *tail), lib)  # noqa: E731

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(k):
            fn()
        b.record(s)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    timed(new, 1)                                               # warm-up (sizes the workspace)
    ok_new = correct(True)
    timed(old, 1)
    ok_old = correct(False)
    t_new, t_old = [], []
    for _ in range(rounds):                                     # interleaved round by round
        t_new.append(timed(new, steps))
        t_old.append(timed(old, steps))
    val.zero_()
    timed(new, 1)
    ok_new = ok_new and correct(True)
    nk = r + 1 if masked else r // 2 + 1
    Tg = group(n, nk, T)
    diff = [a - b for a, b in zip(t_new, t_old)]
    print(json.dumps(dict(host=socket.gethostname(), steps=steps, rounds=rounds, S=S, count=n, degree=t, r=r, what="evaluate_wide",
                          T=T, targets=which, input=inp, erased=n_erased, overwritten=n_over, correct=ok_new, decode_call_correct=ok_old,
                          targets_per_group=Tg, secrets_per_pass_evaluate=passes(S, n, r, nk, Tg), secrets_per_pass_decode=passes(S, n, r, nk),
                          ms_evaluate_call=stats(t_new), ms_decode_call=stats(t_old), ms_difference=stats(diff))), flush=True)
    return 0 if ok_new and ok_old else 1


def run_points(steps, rounds):
    import torch

    import pvw_rs_amd as P
    from pvw_rs_amd import api

    dev = torch.device("cuda", 0)
    N, n, S = 8192, 4096, 64
    p = P.PvwParametersBuilder().set_parties(N).set_dimension(2).set_l(8).set_moduli(MODULI).build()
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    nptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pm = api._wide_modulus(SECP_N)
    ix = np.arange(n, dtype=np.uint64)
    W = (n + 63) // 64
    failed = 0
    for K in (16, 64):
        t = 2048 - K                                            # polynomial degree t + K - 1 = 2047, r = 2048
        rng = np.random.default_rng(K)
        secrets = rng.integers(0, 1 << 63, size=(S, K, 4), dtype=np.uint64)
        d_se = torch.from_numpy(secrets.view(np.int64)).to(dev)
        seeds = rng.integers(0, 256, size=S * 32, dtype=np.uint8)
        dealt = torch.empty((S, N, 4), dtype=torch.int64, device=dev)
        api._check(lib.pvw_shamir_shares_packed_wide_device(p._h, ptr(d_se), S, K, t, nptr(pm), nptr(seeds), None, ptr(dealt), sp), lib)
        s.synchronize()
        order = rng.permutation(n)
        basis = np.ascontiguousarray(ix[:t + K])
        for inp in ("consistent", "1024_overwritten", "1024_erased"):
            n_erased, n_over, masked = INPUTS[inp]
            cols = order[:n_erased + n_over]
            shares = dealt[:, :n].clone()
            if len(cols):
                junk = rng.integers(0, 1 << 63, size=(S, len(cols), 4), dtype=np.int64)
                shares[:, torch.from_numpy(np.sort(cols)).to(dev)] = torch.from_numpy(junk).to(dev)
            er = np.zeros((S, W), dtype=np.uint64)
            for c in order[:n_erased]:
                er[:, c // 64] |= np.uint64(1 << (int(c) % 64))
            d_er = torch.from_numpy(er.view(np.int64)).to(dev) if masked else None
            sec = torch.empty((S, K, 4), dtype=torch.int64, device=dev)
            val = torch.empty((S, t + K, 4), dtype=torch.int64, device=dev)
            nerr = torch.empty(S, dtype=torch.int32, device=dev)
            col = torch.empty(n, dtype=torch.int32, device=dev)
            mask = torch.empty((S, W), dtype=torch.int64, device=dev)
            h_val_t = torch.zeros((S, t + K, 4), dtype=torch.int64).pin_memory()
            h_val = h_val_t.numpy().view(np.uint64)
            h_sec = np.zeros((S, K, 4), dtype=np.uint64)
            report = (ptr(nerr), ptr(col), ptr(mask), sp)

            def new():
                api._check(lib.pvw_shamir_packed_wide_secrets_device(p._h, nptr(pm), K, t, nptr(ix), n, ptr(shares), S, n, 1, ptr(d_er),
                                                                     ptr(sec), *report), lib)

            def old():
                head = (p._h, nptr(pm), t + K - 1, nptr(ix), n, ptr(shares), S, n, 1)
                tail = (nptr(basis), t + K, ptr(val), None, *report)
                if masked:
                    api._check(lib.pvw_shamir_evaluate_wide_erasures_device(*head, ptr(d_er), *tail), lib)
                else:
                    api._check(lib.pvw_shamir_evaluate_wide_corrected_device(*head, *tail), lib)
                with torch.cuda.stream(s):
                    h_val_t.copy_(val, non_blocking=True)
                s.synchronize()
                api._check(lib.pvw_shamir_reconstruct_packed_wide(nptr(pm), K, nptr(basis), nptr(h_val), t + K, S, nptr(h_sec)), lib)

            def timed(fn, k):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(k):
                    fn()
                b.record(s)
                torch.cuda.synchronize()
                return a.elapsed_time(b) / k

            def errs_ok():
                return bool((nerr.cpu().numpy().view(np.uint32) == n_over).all())

            timed(new, 1)                                       # warm-up (sizes the workspace)
            ok_new = errs_ok() and np.array_equal(sec.cpu().numpy().view(np.uint64), secrets)
            timed(old, 1)
            ok_old = errs_ok() and np.array_equal(h_sec, secrets)
            t_new, t_old = [], []
            for _ in range(rounds):                             # interleaved round by round
                t_new.append(timed(new, steps))
                t_old.append(timed(old, steps))
            sec.zero_()
            h_sec[:] = 0
            timed(new, 1)
            timed(old, 1)
            ok_new = ok_new and np.array_equal(sec.cpu().numpy().view(np.uint64), secrets)
            ok_old = ok_old and np.array_equal(h_sec, secrets)
            nk = 2049 if masked else 1025
            print(json.dumps(dict(host=socket.gethostname(), steps=steps, rounds=rounds, S=S, count=n, pack=K, degree=t, r=2048,
                                  what="packed_wide_secrets", input=inp, erased=n_erased, overwritten=n_over, correct=ok_new,
                                  old_route_correct=ok_old, secrets_per_pass_new=passes(S, n, 2048, nk, group(n, nk, K)),
                                  secrets_per_pass_old=passes(S, n, 2048, nk, group(n, nk, t + K)), ms_packed_call=stats(t_new),
                                  ms_old_route=stats(t_old), ratio_of_medians=round(float(np.median(t_old) / np.median(t_new)), 3))),
                  flush=True)
            failed += not (ok_new and ok_old)
    return 1 if failed else 0


def main():
    steps, rounds, limit = int(arg("--steps", 2)), int(arg("--rounds", 5)), int(arg("--limit", 240))
    if "--points" in sys.argv:
        sys.exit(run_points(steps, rounds))
    if "--case" in sys.argv:
        sys.exit(run_case(arg("--case", None), steps, rounds))
    for case in CASES:                                          # a child each, under its own time limit; the first failure ends the run
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--steps", str(steps), "--rounds", str(rounds)],
                                timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": case, "error": f"no result within {limit} s"}), flush=True)
            sys.exit(124)
        if rc != 0:
            print(json.dumps({"case": case, "error": f"exit status {rc}"}), flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()

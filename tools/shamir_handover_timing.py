#!/usr/bin/env python3
"""The one-word handover in one call against the route the library offered before it, on the same buffers,
interleaved round by round in one process on one stream (run on the GPU box under a time limit):
    timeout -k 10 500 python tools/shamir_handover_timing.py [--rounds 5] [--steps 2] [--parties 4096]
One JSON line per (D old holders, T targets) in {256, 1024} x {1, 16}; every figure is the median over the rounds of the mean of
--steps calls between two HIP events, after a warm-up of every side, with the rounds themselves.  Shape: config 3 (n = 4096,
k = 256, l = 8, 17 moduli), p = 2^61 - 1, every fourth holder masked out, uniform random words as ciphertexts (1024 holders are
about 4.8 GB).
  handover   pvw_decrypt_all_handover_device: the mask in device memory, weights on the device, one many-combinations pass
  old_route  pvw_shamir_lagrange_weights_at over the compacted holders on the host, the scatter, the upload of the rows, then
             pvw_decrypt_all_lincomb_many_plain_device (the host's time lies between the two events: the stream waits for it)
  weights    pvw_shamir_handover_weights_device alone
  host_weights_ms  the host's part of old_route alone, by the wall clock"""
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

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402

dev = torch.device("cuda", 0)
PLAIN = (1 << 61) - 1


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rand(*shape):
    return torch.empty(shape, dtype=torch.int64, device=dev).random_()


def timed(fn, steps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, steps, rounds, stream):
    for fn in fns.values():
        timed(fn, 1, stream)
    acc = {name: [] for name in fns}
    for r in range(rounds):
        order = list(fns)
        if r % 2:
            order.reverse()
        for name in order:
            acc[name].append(timed(fns[name], steps, stream))
    return {name: {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                   "rounds_ms": [round(x, 4) for x in v]} for name, v in acc.items()}


def main():
    rounds, steps, NP = int(arg("--rounds", 5)), int(arg("--steps", 2)), int(arg("--parties", 4096))
    n, k, l, L = 4096, 256, 8, 17
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(M.bench_moduli(L)).build()
    lib = _ffi.lib()
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    with torch.cuda.stream(s):
        sk = torch.randint(-1, 2, (NP, k, l), dtype=torch.int64, device=dev)
        for D in (256, 1024):
            c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
            idx = np.arange(D, dtype=np.uint64)
            valid = np.array([d % 4 != 1 for d in range(D)], dtype=np.uint8)
            d_valid = torch.from_numpy(valid).to(dev)
            on = np.flatnonzero(valid)
            vidx = np.ascontiguousarray(idx[on])
            for T in (1, 16):
                targets = np.array([PLAIN - 1 - m for m in range(T)], dtype=np.uint64)
                out, nz = rand(NP, T), rand(NP, T)
                st, cnt = torch.zeros((NP, T), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
                w, w_old = torch.zeros((T, D), dtype=torch.int64, device=dev), torch.zeros((T, D), dtype=torch.int64, device=dev)
                comp, rows = np.zeros((T, len(on)), dtype=np.int64), np.zeros((T, D), dtype=np.int64)
                pinned = torch.zeros((T, D), dtype=torch.int64).pin_memory()

                def handover():
                    p._call("pvw_decrypt_all_handover_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, ptr(d_valid), api._ptr(idx), api._ptr(targets),
                            T, P.REPR_NTT, ptr(out), ptr(nz), ptr(st), ptr(cnt), PLAIN, 0, None, sp)

                def host_weights():
                    api._check(lib.pvw_shamir_lagrange_weights_at(PLAIN, api._ptr(vidx), len(vidx), api._ptr(targets), T, api._ptr(comp)), lib)
                    rows[:, on] = comp
                    pinned.copy_(torch.from_numpy(rows))

                def old_route():
                    host_weights()
                    w_old.copy_(pinned, non_blocking=True)
                    p._call("pvw_decrypt_all_lincomb_many_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, ptr(d_valid), ptr(w_old), T,
                            P.REPR_NTT, ptr(out), ptr(nz), ptr(st), None, PLAIN, 0, None, sp)

                def weights():
                    p._call("pvw_shamir_handover_weights_device", PLAIN, api._ptr(idx), ptr(d_valid), D, api._ptr(targets), T, ptr(w), ptr(cnt), sp)

                res = interleaved({"handover": handover, "old_route": old_route, "weights": weights}, steps, rounds, s)
                assert torch.equal(w, w_old) and cnt.item() == len(on)      # the two routes made the same rows
                t0 = time.perf_counter()
                for _ in range(5):
                    host_weights()
                host_ms = (time.perf_counter() - t0) / 5 * 1e3
                print(json.dumps(dict(case="one-word handover, config 3", holders=D, valid=int(len(on)), targets=T, parties=NP, n=n, k=k, l=l, L=L,
                                      plain_modulus=PLAIN, steps=steps, rounds=rounds, ciphertext_bytes=8 * L * l * D * (k + n),
                                      old_route_over_handover=round(res["old_route"]["ms"] / res["handover"]["ms"], 3),
                                      host_weights_ms=round(host_ms, 4), host=socket.gethostname(), **res)), flush=True)
            del c1, c2


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Encrypt from a seed (PVW_RND_SEED, key in the kernel arguments) against encrypt from a device randomness state
(pvw_rnd_state: keys derived on the device, counter advanced there), interleaved in one process (run on the GPU box):
    python tools/device_rnd_timing.py [--steps 200] [--rounds 5]
Two cases at the config-3 geometry (n = 4096, k = 256, l = 8, 17 limbs), after pvw_prepare:
  single   pvw_encrypt_device vs pvw_encrypt_rs_device
  multi64  pvw_encrypt_multi_device vs pvw_encrypt_multi_rs_device with 64 dealers
Per round, each mode runs --steps back-to-back calls on one stream between two HIP events; the modes alternate within the
round (which one goes first alternates too).  One JSON line per case: median ms per call of each mode over the rounds, and
the ratio state / seed."""
import ctypes as C
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: E402

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi  # noqa: E402

dev = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32


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
    steps, rounds = int(arg("--steps", 200)), int(arg("--rounds", 5))
    n, k, l, L = 4096, 256, 8, 17
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(M.bench_moduli(L)).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    lib = p._lib
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    p.prepare(P.PREPARE_PACKED | P.PREPARE_MFMA, s.cuda_stream)
    st = P.DeviceRandomness(p, SEED, 0)
    rnd = _ffi.pvw_randomness_t()
    rnd.mode = _ffi.RND_SEED
    C.memmove(rnd.seed, SEED, 32)
    D = 64
    sc = torch.from_numpy(np.random.default_rng(1).integers(0, 1 << 32, size=(D, n), dtype=np.uint64).view(np.int64)).to(dev)
    c1 = torch.empty((D, k, L, l), dtype=torch.int64, device=dev)
    c2 = torch.empty((D, n, L, l), dtype=torch.int64, device=dev)
    seeds = np.frombuffer(SEED * D, dtype=np.uint8).copy()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    cases = {
        "single": (lambda: P.api._check(lib.pvw_encrypt_device(p._h, ptr(sc), n, C.byref(rnd), ptr(c1), ptr(c2), P.REPR_NTT, sp), lib),
                   lambda: P.api._check(lib.pvw_encrypt_rs_device(p._h, ptr(sc), n, st._h, ptr(c1), ptr(c2), P.REPR_NTT, sp), lib)),
        "multi64": (lambda: P.api._check(lib.pvw_encrypt_multi_device(p._h, ptr(sc), D, n, seeds.ctypes.data_as(C.c_void_p), ptr(c1),
                                                                      ptr(c2), P.REPR_NTT, sp), lib),
                    lambda: P.api._check(lib.pvw_encrypt_multi_rs_device(p._h, ptr(sc), D, n, st._h, ptr(c1), ptr(c2), P.REPR_NTT,
                                                                         sp), lib)),
    }
    for name, (seed_fn, state_fn) in cases.items():
        case_steps = steps if name == "single" else max(steps // 4, 10)
        for fn in (seed_fn, state_fn):          # warm-up
            timed(fn, 5, s)
        t_seed, t_state = [], []
        for r in range(rounds):
            order = [(seed_fn, t_seed), (state_fn, t_state)]
            if r % 2:
                order.reverse()
            for fn, acc in order:
                acc.append(timed(fn, case_steps, s))
        ms_seed, ms_state = float(np.median(t_seed)), float(np.median(t_state))
        print(json.dumps({"case": name, "n": n, "k": k, "l": l, "L": L, "dealers": D if name == "multi64" else 1,
                          "steps": case_steps, "rounds": rounds, "ms_seed": round(ms_seed, 4), "ms_state": round(ms_state, 4),
                          "ratio_state_seed": round(ms_state / ms_seed, 4), "seed_rounds_ms": [round(x, 4) for x in t_seed],
                          "state_rounds_ms": [round(x, 4) for x in t_state], "host": socket.gethostname()}), flush=True)
    st.free()


if __name__ == "__main__":
    main()

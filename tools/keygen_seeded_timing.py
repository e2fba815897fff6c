#!/usr/bin/env python3
"""Key generation from a seed against key generation from host keys, interleaved in one process after warm-up
(run on the GPU box):
    python tools/keygen_seeded_timing.py [--steps 3] [--rounds 7] [--only c3|k512]
Three synchronous calls over all parties:
  pageable  pvw_keygen from pageable numpy keys (what bench.py --path keygen does)
  pinned    pvw_keygen from pvw_host_alloc memory
  seeded    pvw_keygen_seeded (no keys on the host; left out where the library lacks it, so that an earlier commit can be
            measured with this file)
at the config-3 key-generation workload (n = 4096, k = 256, l = 8, 17 limbs: 67 MB of keys) and at k = 512, l = 16 (n = 4096,
34 limbs: 268 MB of keys).  Per round each call runs --steps times, each timed on the host from entry to return; the order
rotates from round to round.  One JSON line per geometry: wall ms per call as the median of the rounds' means, the rounds'
lowest and highest, and from one profiled call each the context's "keygen" kernel time (the compute, without the upload)."""
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

import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import workloads as W  # noqa: E402

GEOMETRIES = {"c3": (4096, 256, 8, 17), "k512": (4096, 512, 16, 34)}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    steps, rounds, only = int(arg("--steps", 3)), int(arg("--rounds", 7)), arg("--only", None)
    for config, (n, k, l, L) in GEOMETRIES.items():
        if only and config != only:
            continue
        p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(W.bench_moduli(L)).build()
        P.PvwCrs.new_deterministic(p, W.SEED_A)
        lib, h = p._lib, p._h
        ok = lambda rc: P.api._check(rc, lib)  # noqa: E731
        sk_seed, seed = np.frombuffer(W.SEED_ENC, dtype=np.uint8).copy(), np.frombuffer(W.SEED_B, dtype=np.uint8).copy()
        skp, sdp = sk_seed.ctypes.data_as(C.c_void_p), seed.ctypes.data_as(C.c_void_p)
        sk = np.zeros((n, k, l), dtype=np.int64)
        ok(lib.pvw_sample_secret_keys(h, skp, 0, n, sk.ctypes.data_as(C.c_void_p)))
        pinned = C.c_void_p()
        ok(lib.pvw_host_alloc(sk.nbytes, C.byref(pinned)))
        C.memmove(pinned, sk.ctypes.data, sk.nbytes)
        calls = {"pageable": lambda: ok(lib.pvw_keygen(h, 0, n, sk.ctypes.data_as(C.c_void_p), None, sdp)),
                 "pinned": lambda: ok(lib.pvw_keygen(h, 0, n, pinned, None, sdp))}
        if hasattr(lib, "pvw_keygen_seeded"):
            calls["seeded"] = lambda: ok(lib.pvw_keygen_seeded(h, 0, n, skp, sdp))
        names = list(calls)

        def wall(fn):
            torch.cuda.synchronize()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                fn()                                       # synchronous: B-hat is resident and the keys are wiped on return
                t.append((time.perf_counter() - t0) * 1e3)
            return float(np.mean(t))

        rows = {}
        for name in names:                                 # warm-up; the three forms leave the same B-hat
            calls[name]()
            calls[name]()
            row = np.zeros((2, k, L, l), dtype=np.uint64)
            ok(lib.pvw_get_pk(h, n - 2, n, row.ctypes.data_as(C.c_void_p), P.REPR_NTT))
            rows[name] = row
        assert all(np.array_equal(rows[name], rows[names[0]]) for name in names)
        acc = {name: [] for name in names}
        for r in range(rounds):
            q = r % len(names)
            for name in names[q:] + names[:q]:
                acc[name].append(wall(calls[name]))
        kern = {}
        p.set_profiling(True)
        for name in names:
            p.reset_profiling()
            calls[name]()
            torch.cuda.synchronize()
            kern[name] = round(p.kernel_time("keygen")[0], 4)
        p.set_profiling(False)
        ok(lib.pvw_host_free(pinned))
        med = {name: float(np.median(v)) for name, v in acc.items()}
        print(json.dumps({"config": config, "n": n, "k": k, "l": l, "L": L, "key_bytes": int(sk.nbytes), "steps": steps, "rounds": rounds,
                          "wall_ms": {name: round(med[name], 4) for name in names},
                          "wall_ms_low_high": {name: [round(min(v), 4), round(max(v), 4)] for name, v in acc.items()},
                          "keygen_kernel_ms": kern,
                          "rounds_ms": {name: [round(x, 4) for x in v] for name, v in acc.items()},
                          "host": socket.gethostname()}), flush=True)
        sk.fill(0)
        del p


if __name__ == "__main__":
    main()

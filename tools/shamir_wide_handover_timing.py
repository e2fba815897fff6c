#!/usr/bin/env python3
"""The wide handover in one call against the route the library offered before it, on the same buffers, interleaved
round by round in one process on one stream (run on the GPU box under a time limit):
    timeout -k 10 500 python tools/shamir_wide_handover_timing.py [--rounds 5] [--steps 2] [--dealers 192] [--parties 4096]
One JSON line per digit width (64 and 60); every figure is the median over the rounds of the mean of --steps calls between two HIP
events, after a warm-up of every side, with the rounds themselves.  Shape: config 3 (n = 4096, k = 256, l = 8, 17 moduli), the
secp256k1 order, 52-bit limbs, D old holders (D * 5 vectors; 192 holders are about 4.5 GB of ciphertexts), uniform random words.
  handover   pvw_decrypt_all_handover_wide_device: weights, 5 combined ciphertexts, 5 decrypts a party, the fold
  long_way   pvw_decrypt_all_plain_device of all D * 5 vectors, pvw_shamir_wide_from_limbs_device in place,
             pvw_shamir_reconstruct_wide_checked_device with strides (1, D) at degree D - 1
  weights    pvw_shamir_wide_handover_weights_device alone
  fold       pvw_shamir_wide_from_digits_device alone over a [P][5] report"""
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
from pvw_rs_amd import api  # noqa: E402

dev = torch.device("cuda", 0)
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


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
    rounds, steps = int(arg("--rounds", 5)), int(arg("--steps", 2))
    D, NP = int(arg("--dealers", 192)), int(arg("--parties", 4096))
    n, k, l, L, lb = 4096, 256, 8, 17, 52
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(M.bench_moduli(L)).build()
    pm = api._wide_modulus(SECP_N)
    NL = P.shamir_wide_limbs(SECP_N, lb)
    s = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(s.cuda_stream)
    idx = np.arange(D, dtype=np.uint64)
    with torch.cuda.stream(s):
        c1, c2 = rand(D * NL, k, L, l), rand(D * NL, n, L, l)
        sk = torch.randint(-1, 2, (NP, k, l), dtype=torch.int64, device=dev)
        out, st, cnt = rand(NP, 1, 4), torch.zeros((NP, 1), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        limbs, nz, st2 = rand(NP, D * NL), rand(NP, D * NL), torch.zeros((NP, D * NL), dtype=torch.int32, device=dev)
        wide_sh, sec, bad, colbad = rand(NP, D, 4), rand(NP, 4), torch.zeros(NP, dtype=torch.int32, device=dev), torch.zeros(D, dtype=torch.int32, device=dev)
        for b in (64, 60):
            V = P.shamir_wide_handover_shape(SECP_N, lb, b)[1]
            w = torch.zeros((V, D * NL), dtype=torch.int64, device=dev)
            rep_w, rep_s = rand(NP, V, 2), torch.zeros((NP, V), dtype=torch.int32, device=dev)

            def handover():
                p._call("pvw_decrypt_all_handover_wide_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, api._ptr(pm), lb, b, api._ptr(idx), None, None,
                        1, P.REPR_NTT, ptr(out), ptr(st), ptr(cnt), sp)

            def long_way():
                p._call("pvw_decrypt_all_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D * NL, P.REPR_NTT, ptr(limbs), ptr(nz), ptr(st2), 0, 0,
                        None, sp)
                p._call("pvw_shamir_wide_from_limbs_device", api._ptr(pm), ptr(limbs), NP * D, 1, NL, lb, NL, ptr(wide_sh), sp)
                p._call("pvw_shamir_reconstruct_wide_checked_device", api._ptr(pm), D - 1, api._ptr(idx), D, ptr(wide_sh), NP, D, 1, ptr(sec),
                        ptr(bad), ptr(colbad), sp)

            def weights():
                p._call("pvw_shamir_wide_handover_weights_device", api._ptr(pm), api._ptr(idx), None, D, None, 1, lb, b, ptr(w), sp)

            def fold():
                p._call("pvw_shamir_wide_from_digits_device", api._ptr(pm), b, V, ptr(rep_w), ptr(rep_s), 2, NP, ptr(out), ptr(st), sp)

            res = interleaved({"handover": handover, "long_way": long_way, "weights": weights, "fold": fold}, steps, rounds, s)
            print(json.dumps(dict(case="wide handover, config 3", digit_bits=b, num_digits=V, dealers=D, vectors=D * NL, parties=NP, n=n, k=k, l=l,
                                  L=L, limb_bits=lb, steps=steps, rounds=rounds, ciphertext_bytes=8 * L * l * D * NL * (k + n),
                                  long_way_over_handover=round(res["long_way"]["ms"] / res["handover"]["ms"], 3), host=socket.gethostname(),
                                  **res)), flush=True)


if __name__ == "__main__":
    main()

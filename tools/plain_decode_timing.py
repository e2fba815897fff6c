#!/usr/bin/env python3
"""The plain decode against the checked decode it extends, interleaved in one process on one stream (run on the
GPU box):
    python tools/plain_decode_timing.py [--rounds 7] [--steps 20]
One JSON line per case; every figure is the median over the rounds of the mean of --steps calls between two HIP events, after
warm-up, the order alternating from round to round.  The yardstick is the checked side of the same run.
  decode   pvw_decode_plain_device (modulus = the first limb, wide_words = W) against pvw_decode_checked_device on the SAME
           buffers: the config-5 shard (D = 1024, l = 16, 34 moduli), honest residues (m Delta^j + small noise, shares uniform
           below the first limb times a 40-dealer sum) and uniform residues
  all_sum  pvw_decrypt_all_sum_plain_device against pvw_decrypt_all_sum_checked_device, config 3 (k = 256, l = 8, 17 moduli),
           P = D = 1024, uniform words, after pvw_prepare(PVW_PREPARE_SUM)"""
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

dev = torch.device("cuda", 0)


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
    for fn in fns:
        timed(fn, 3, stream)
    acc = [[] for _ in fns]
    for r in range(rounds):
        order = list(range(len(fns)))
        if r % 2:
            order.reverse()
        for i in order:
            acc[i].append(timed(fns[i], steps, stream))
    return acc


def report(case, acc, count, **kw):
    """both sides, the checked side's own spread, the difference and what it comes to per ciphertext"""
    chk, pln = acc
    m_chk, m_pln = float(np.median(chk)), float(np.median(pln))
    spread = max(chk) - min(chk)
    diff = m_pln - m_chk
    print(json.dumps(dict(kw, case=case, ms_checked=round(m_chk, 5), ms_plain=round(m_pln, 5), checked_rounds_ms=[round(x, 5) for x in chk],
                          plain_rounds_ms=[round(x, 5) for x in pln], checked_spread_ms=round(spread, 5), diff_ms=round(diff, 5),
                          diff_ns_per_ciphertext=round(diff * 1e6 / count, 2), inside_checked_spread=bool(abs(diff) <= spread),
                          host=socket.gethostname())), flush=True)


def params(n, k, l, L):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(M.bench_moduli(L)).build()


def decode_case(steps, rounds, s):
    l, L, D = 16, 34, 1024
    moduli = M.bench_moduli(L)
    p = params(2, 512, l, L)
    m = M.Params(2, 512, l, moduli)
    W = (m.Q.bit_length() + 63) // 64
    q0 = int(moduli[0])
    rng = np.random.default_rng(1)
    honest = np.zeros((D, L, l), dtype=np.uint64)
    for d in range(D):
        msg = sum(int(x) for x in rng.integers(0, q0, 40))
        z = [(-(msg * m.delta ** j) + int(rng.integers(-10 ** 6, 10 ** 6))) % m.Q for j in range(l)]
        honest[d] = [[v % q for v in z] for q in moduli]
    sp = C.c_void_p(s.cuda_stream)
    out, ns, st, wd = rand(D), rand(D), torch.zeros(D, dtype=torch.int32, device=dev), rand(D, W)
    for name, nz in (("honest", torch.from_numpy(honest.view(np.int64)).to(dev)), ("uniform", rand(D, L, l))):
        checked = lambda: p._call("pvw_decode_checked_device", ptr(nz), D, ptr(out), ptr(ns), ptr(st), sp)                # noqa: E731
        plain = lambda: p._call("pvw_decode_plain_device", ptr(nz), D, ptr(out), ptr(ns), ptr(st), q0, W, ptr(wd), sp)   # noqa: E731
        report("decode c5shard " + name, interleaved([checked, plain], steps, rounds, s), D, dealers=D, l=l, L=L, wide_words=W,
               steps=steps, rounds=rounds)


def all_sum_case(steps, rounds, s):
    n, k, l, L, NP, D = 1024, 256, 8, 17, 1024, 1024
    p = params(n, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    W = (p.q_total().bit_length() + 63) // 64
    q0 = int(p.moduli()[0])
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    sk = torch.randint(-1, 2, (NP, k, l), dtype=torch.int64, device=dev)
    out, ns, st, wd = rand(NP), rand(NP), torch.zeros(NP, dtype=torch.int32, device=dev), rand(NP, W)
    checked = lambda: p._call("pvw_decrypt_all_sum_checked_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, None, P.REPR_NTT, ptr(out),   # noqa: E731
                              ptr(ns), ptr(st), None, sp)
    plain = lambda: p._call("pvw_decrypt_all_sum_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, None, P.REPR_NTT, ptr(out),       # noqa: E731
                            ptr(ns), ptr(st), None, q0, W, ptr(wd), sp)
    report("decrypt_all_sum config 3", interleaved([checked, plain], steps, rounds, s), NP, parties=NP, dealers=D, k=k, l=l, L=L,
           wide_words=W, steps=steps, rounds=rounds)


def main():
    rounds, steps = int(arg("--rounds", 7)), int(arg("--steps", 20))
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        decode_case(steps, rounds, s)
        all_sum_case(max(steps // 2, 2), rounds, s)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Many weighted sums of the same dealers' ciphertexts against what a caller did before them -- R calls of the
single-combination entry point on the same buffers -- interleaved in one process on one stream (run on the GPU box, every step
under a time limit of its own, chained, nothing tried twice):
    timeout -k 10 400 python tools/ct_lincomb_many_timing.py --tuning --only device && \
    timeout -k 10 300 python tools/ct_lincomb_many_timing.py --only all && timeout -k 10 300 python tools/ct_lincomb_many_timing.py --only hostbuf
    [--rounds 5] [--steps 4]
One JSON line per case; every figure is the median over the rounds of the mean of --steps calls between two HIP events, after a
warm-up of every side; `spread` is (max - min) / median of a side's rounds.  Uniform random words, field-sized weights (centred
in a 61-bit field, no zeros), after pvw_prepare(PVW_PREPARE_SUM).
  device    pvw_ct_lincomb_many_device against R calls of pvw_ct_lincomb_device, R in {1, 2, 4, 8, 16, 64}, D = 1024: the
            config-3 whole-row shape (k = 256, l = 8, 17 moduli, n = 4096) and the config-5 shard column shape (k = 512, l = 16,
            34 moduli, one row); with --tuning every row tile PVW_SUM_RT = 2 / 4 / 8 is a side of its own, without it the
            shipped tile is the only one
  all       pvw_decrypt_all_lincomb_many_plain_device at P = D = 1024, R = 16 (config 3) against 16 calls of
            pvw_decrypt_all_lincomb_plain_device
  grid      (only when asked for) the config-3 polynomials with 512 / 1024 / 2048 / 3072 rows at R = 16: the grids between the two
            shapes above, where the shipped row tile changes (ct_lincomb_many_tile)
  hostbuf   pvw_ct_lincomb_many at D = 128, R = 16 (config-3 polynomials, n = 1024) against 16 calls of pvw_ct_lincomb"""
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
PLAIN = (1 << 61) - 1


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def nptr(a):
    return a.ctypes.data_as(C.c_void_p)


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
    """{name: (median ms per call, spread, rounds)} of each side, the order alternating from round to round"""
    for fn in fns.values():
        timed(fn, 1, stream)
    acc = {name: [] for name in fns}
    for r in range(rounds):
        order = list(fns)
        if r % 2:
            order.reverse()
        for name in order:
            acc[name].append(timed(fns[name], steps, stream))
    out = {}
    for name, v in acc.items():
        med = float(np.median(v))
        out[name] = {"ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4), "rounds_ms": [round(x, 4) for x in v]}
    return out


def params(n, k, l, L):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(M.bench_moduli(L)).build()


def emit(**kw):
    print(json.dumps(dict(kw, host=socket.gethostname())), flush=True)


def field_weights(R, D):
    w = np.random.default_rng(R * 4099 + D).integers(-(PLAIN // 2), PLAIN // 2, (R, D), dtype=np.int64, endpoint=True)
    w[w == 0] = 1
    return w


def with_tile(rt, fn):
    def run():
        os.environ["PVW_SUM_RT"] = str(rt)              # read per call by the tuning build; the shipped library has no such switch
        fn()
    return run


def device_case(name, n, k, l, L, D, rows, combos, tiles, steps, rounds, s):
    p = params(n, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    Rmax = max(combos)
    o1, o2, cnt = rand(Rmax, k, L, l), rand(Rmax, rows, L, l), torch.zeros(Rmax, dtype=torch.int32, device=dev)
    for R in combos:
        w = torch.from_numpy(field_weights(R, D)).to(dev)
        wr, a1, a2 = [w[r] for r in range(R)], [o1[r] for r in range(R)], [o2[r] for r in range(R)]

        def singles():
            for r in range(R):
                p._call("pvw_ct_lincomb_device", ptr(c1), ptr(c2), D, None, ptr(wr[r]), 0, rows, ptr(a1[r]), ptr(a2[r]), None, sp)

        many = lambda: p._call("pvw_ct_lincomb_many_device", ptr(c1), ptr(c2), D, None, ptr(w), R, 0, rows, ptr(o1), ptr(o2), ptr(cnt), sp)  # noqa: E731
        fns = {"singles": singles}
        for rt in tiles:
            fns["many" if rt is None else f"many_rt{rt}"] = many if rt is None else with_tile(rt, many)
        st = max(1, steps // max(1, R // 8))
        res = interleaved(fns, st, rounds, s)
        ratio = {nm: round(res["singles"]["ms"] / res[nm]["ms"], 3) for nm in res if nm != "singles"}
        emit(case="device " + name, n=n, k=k, l=l, L=L, dealers=D, rows=rows, combos=R, steps=st, rounds=rounds,
             bytes_one_pass=8 * L * l * D * (k + rows), speedup_over_singles=ratio, **res)


def all_case(NP, R, steps, rounds, s):
    n, k, l, L = 4096, 256, 8, 17
    D = NP
    p = params(n, k, l, L)
    p.prepare(P.PREPARE_SUM, s.cuda_stream)
    sp = C.c_void_p(s.cuda_stream)
    c1, c2 = rand(D, k, L, l), rand(D, n, L, l)
    sk = torch.randint(-1, 2, (NP, k, l), dtype=torch.int64, device=dev)
    w = torch.from_numpy(field_weights(R, D)).to(dev)
    out, ns, st = rand(NP, R), rand(NP, R), torch.zeros((NP, R), dtype=torch.int32, device=dev)
    o1 = [rand(NP) for _ in range(R)]
    n1, s1 = rand(NP), torch.zeros(NP, dtype=torch.int32, device=dev)
    wr = [w[r] for r in range(R)]

    def singles():
        for r in range(R):
            p._call("pvw_decrypt_all_lincomb_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, None, ptr(wr[r]), P.REPR_NTT, ptr(o1[r]),
                    ptr(n1), ptr(s1), None, PLAIN, 0, None, sp)

    many = lambda: p._call("pvw_decrypt_all_lincomb_many_plain_device", 0, NP, ptr(sk), ptr(c1), ptr(c2), D, None, ptr(w), R, P.REPR_NTT,  # noqa: E731
                           ptr(out), ptr(ns), ptr(st), None, PLAIN, 0, None, sp)
    res = interleaved({"singles": singles, "many": many}, steps, rounds, s)
    same = all(torch.equal(out[:, r], o1[r]) for r in range(R))
    emit(case="all", parties=NP, dealers=D, combos=R, n=n, k=k, l=l, L=L, steps=steps, rounds=rounds, results_equal=same,
         speedup_over_singles=round(res["singles"]["ms"] / res["many"]["ms"], 3), **res)


def hostbuf_case(D, R, steps, rounds, s):
    n, k, l, L = 1024, 256, 8, 17
    p = params(n, k, l, L)
    rng = np.random.default_rng(D)
    c1 = rng.integers(0, 1 << 62, (D, k, L, l), dtype=np.uint64)
    c2 = rng.integers(0, 1 << 62, (D, n, L, l), dtype=np.uint64)
    w = field_weights(R, D)
    o1, o2 = np.zeros((R, k, L, l), np.uint64), np.zeros((R, n, L, l), np.uint64)

    def singles():
        for r in range(R):
            p._call("pvw_ct_lincomb", nptr(c1), nptr(c2), D, None, nptr(w[r]), 0, n, nptr(o1[r]), nptr(o2[r]), None)

    many = lambda: p._call("pvw_ct_lincomb_many", nptr(c1), nptr(c2), D, None, nptr(w), R, 0, n, nptr(o1), nptr(o2), None)  # noqa: E731
    res = interleaved({"singles": singles, "many": many}, steps, rounds, s)
    emit(case="hostbuf", dealers=D, combos=R, n=n, k=k, l=l, L=L, steps=steps, rounds=rounds, upload_bytes=int(c1.nbytes + c2.nbytes),
         speedup_over_singles=round(res["singles"]["ms"] / res["many"]["ms"], 3), **res)


def main():
    rounds, steps = int(arg("--rounds", 5)), int(arg("--steps", 4))
    only = arg("--only", "")
    tiles = [None]
    if "--tuning" in sys.argv:              # the measurement build: PVW_SUM_RT selects the row tile
        from pvw_rs_amd import _ffi
        _ffi.select("tuning")
        tiles = [2, 4, 8]
    combos = [int(x) for x in arg("--combos", "1,2,4,8,16,64").split(",")]
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        if only in ("", "device"):
            device_case("config-5 shard, column form", 1, 512, 16, 34, 1024, 1, combos, tiles, steps, rounds, s)
            device_case("config 3, whole rows", 4096, 256, 8, 17, 1024, 4096, combos, tiles, steps, rounds, s)
        if only == "grid":                  # where the row tile changes: grids between the two shapes above, R = 16 only
            for rows in (512, 1024, 2048, 3072):
                device_case(f"config 3, {rows} rows", 4096, 256, 8, 17, 1024, rows, [16], tiles, steps, rounds, s)
        if only in ("", "all"):
            all_case(1024, 16, max(steps // 2, 1), rounds, s)
        if only in ("", "hostbuf"):
            hostbuf_case(128, 16, 1, min(rounds, 3), s)


if __name__ == "__main__":
    main()

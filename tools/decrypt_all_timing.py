#!/usr/bin/env python3
"""pvw_decrypt_all_device against the loop over pvw_decrypt_batch_device_sk it replaces (run on the GPU box):
    python tools/decrypt_all_timing.py [--cases 64,256,1024,4096] [--steps 5] [--tuning]
One JSON line per case: P = D at the config-3 geometry (k = 256, l = 8, 17 limbs) and P = D = 1024 on the reference's
128-bit set (4 x 56-bit moduli, k = 1024, l = 8).  Ciphertexts are made on the device (pvw_keygen, pvw_encrypt_multi_device).
  ms_call        HIP-event time per pvw_decrypt_all_device call (median of --steps after a warm-up call)
  split_ms       per-call device time of its kernels by pvw_ctx_kernel_time (profiled run of its own)
  loop_ms        the per-party loop for the same parties: pvw_decrypt_batch_device_sk with each party's key resident (loaded
                 outside the timing) and its c2 column gathered outside the timing; over all parties when P <= 256, else over
                 a seeded sample of 64 parties scaled by P / 64 (loop_sampled says which)
  i8_tops        2 x 64 x P_pad x D x k x L x l / GEMM time (8 x 8 byte-digit products per element pair), against 5 POP/s
  finish_tbs     (intermediate in + c2 in + noisy out) bytes / finish time, against 8 TB/s
--threshold (measurement build): P in {2, 4, 8, 16, 32, 64} parties against D = 1024 dealers at config 3, each side of
the dispatch forced through PVW_DECRYPT_ALL_MIN_PARTIES (1: matrix cores, 2^30: party by party), one JSON line per P."""
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

if "--tuning" in sys.argv or "--threshold" in sys.argv:
    _ffi.select("tuning")

dev = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def events_ms(fn, steps):
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def case(name, n, k, l, moduli, steps):
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()
    L = len(moduli)
    crs = P.PvwCrs.new_deterministic(p, SEED)
    P.GlobalPublicKey.new(crs)
    seed = np.frombuffer(SEED, dtype=np.uint8).copy()
    sk = np.zeros((n, k, l), dtype=np.int64)
    p._call("pvw_sample_secret_keys", seed.ctypes.data, 0, n, sk.ctypes.data)
    p._call("pvw_keygen", 0, n, sk.ctypes.data, None, seed.ctypes.data)
    scalars = np.random.default_rng(1).integers(0, 1 << 32, size=(n, n), dtype=np.uint64)
    t_sc = torch.from_numpy(scalars.view(np.int64)).to(dev)
    t_c1 = torch.empty((n, k, L, l), dtype=torch.int64, device=dev)
    t_c2 = torch.empty((n, n, L, l), dtype=torch.int64, device=dev)
    t_sk = torch.from_numpy(sk).to(dev)
    t_out = torch.zeros((n, n), dtype=torch.int64, device=dev)
    seeds = np.zeros(n * 32, dtype=np.uint8)
    seeds[::32] = np.arange(n) & 0xFF
    seeds[1::32] = np.arange(n) >> 8
    torch.cuda.synchronize()
    p._call("pvw_encrypt_multi_device", t_sc.data_ptr(), n, n, seeds.ctypes.data, t_c1.data_ptr(), t_c2.data_ptr(), P.REPR_NTT, None)
    p.synchronize()
    stream = torch.cuda.current_stream().cuda_stream      # a stream of our own (main): the events are recorded on it

    def call():
        p._call("pvw_decrypt_all_device", 0, n, t_sk.data_ptr(), t_c1.data_ptr(), t_c2.data_ptr(), n, P.REPR_NTT, t_out.data_ptr(),
                C.c_void_p(stream))
    call()
    torch.cuda.synchronize()
    ok = float((t_out.cpu().numpy().view(np.uint64) == scalars.T).mean())
    ms = events_ms(call, steps)
    p.reset_profiling()
    p.set_profiling(True)
    call()
    torch.cuda.synchronize()
    split = {kn: round(p.kernel_time(kn)[0], 4) for kn in ("prep", "digits", "gemm", "finish", "intt", "decode")}
    p.set_profiling(False)
    # the per-party loop with resident keys
    sample = np.arange(n) if n <= 256 else np.sort(np.random.default_rng(7).choice(n, 64, replace=False))
    cols = {int(i): t_c2[:, i].contiguous() for i in sample}
    keys = {int(i): P.SecretKey.from_coefficients(p, sk[i]).load_device() for i in sample}
    t_nz = torch.empty((n, L, l), dtype=torch.int64, device=dev)
    t_o = torch.empty(n, dtype=torch.int64, device=dev)

    def loop():
        for i in sample:
            p._call("pvw_decrypt_batch_device_sk", keys[int(i)]._h, t_c1.data_ptr(), cols[int(i)].data_ptr(), n, P.REPR_NTT,
                    t_nz.data_ptr(), t_o.data_ptr(), C.c_void_p(stream))
    loop()
    torch.cuda.synchronize()
    loop_ms = events_ms(loop, max(1, min(steps, 3))) * n / len(sample)
    for key in keys.values():
        key.free()
    rows_pad = -(-n // 128) * 128
    ops = 2.0 * 64 * rows_pad * n * k * L * l
    fin_bytes = 3.0 * n * n * L * l * 8
    res = {"case": name, "P": n, "D": n, "k": k, "l": l, "L": L, "ms_call": round(ms, 3), "split_ms": split,
           "loop_ms": round(loop_ms, 2), "loop_sampled": len(sample) < n, "speedup": round(loop_ms / ms, 2),
           "i8_tops": round(ops / (split["gemm"] * 1e-3) / 1e12, 1) if split["gemm"] else None,
           "i8_frac_of_5000": round(ops / (split["gemm"] * 1e-3) / 5e15, 3) if split["gemm"] else None,
           "finish_tbs": round(fin_bytes / (split["finish"] * 1e-3) / 1e12, 2) if split["finish"] else None,
           "finish_frac_of_8": round(fin_bytes / (split["finish"] * 1e-3) / 8e12, 3) if split["finish"] else None,
           "dealt_match": round(ok, 6), "host": socket.gethostname(), "tuning": _ffi.lib().pvw_build_is_tuning() == 1}
    print(json.dumps(res), flush=True)
    del t_c1, t_c2, cols
    torch.cuda.empty_cache()


def threshold(steps, D=1024):
    n, k, l, moduli = D, 256, 8, M.bench_moduli(17)
    p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()
    L = len(moduli)
    g = torch.Generator(device=dev).manual_seed(3)
    q = torch.tensor(moduli, dtype=torch.int64, device=dev).view(1, 1, L, 1)
    t_c1 = torch.randint(0, 1 << 62, (D, k, L, l), generator=g, device=dev) % q
    t_c2 = torch.randint(0, 1 << 62, (D, n, L, l), generator=g, device=dev) % q
    t_sk = torch.randint(-1, 2, (64, k, l), generator=g, device=dev)
    t_out = torch.zeros((64, D), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    for np_ in (2, 4, 8, 16, 32, 64):
        row = {"case": "threshold_config3_D1024", "P": np_, "D": D}
        outs = []
        for side, env in (("gemm_ms", "1"), ("per_party_ms", str(1 << 30))):
            os.environ["PVW_DECRYPT_ALL_MIN_PARTIES"] = env
            def call():
                p._call("pvw_decrypt_all_device", 0, np_, t_sk.data_ptr(), t_c1.data_ptr(), t_c2.data_ptr(), D, P.REPR_NTT,
                        t_out.data_ptr(), C.c_void_p(stream))
            call()
            torch.cuda.synchronize()
            row[side] = round(events_ms(call, steps), 3)
            outs.append(t_out[:np_].clone())
        row["equal"] = bool(torch.equal(outs[0], outs[1]))
        row["host"] = socket.gethostname()
        print(json.dumps(row), flush=True)
    os.environ.pop("PVW_DECRYPT_ALL_MIN_PARTIES", None)


def main():
    steps = int(arg("--steps", "5"))
    # every call and every event on one non-default stream (a NULL stream would send the library to its own stream,
    # which the events would not wait for)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(steps)
    torch.cuda.synchronize()


def run(steps):
    if "--threshold" in sys.argv:
        threshold(steps)
        return
    for s in arg("--cases", "64,256,1024,4096").split(","):
        if s:
            case(f"config3_P{s}", int(s), 256, 8, M.bench_moduli(17), steps)
    if "--no-128" not in sys.argv:
        case("sec128_P1024", 1024, 1024, 8, [0x800000022A0001, 0x800000021A0001, 0x80000002120001, 0x80000001F60001], steps)


if __name__ == "__main__":
    main()

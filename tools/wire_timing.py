"""Wire format v1: device time of wire_pack_kernel / wire_unpack_kernel (HIP events around the launches, after
warm-up, same process) in GB/s of bytes read plus written, on the config-3 public key (4096 x 256 polynomials, l = 8, 17
61-bit moduli: 1.14 GB of words) and on a 64-dealer ciphertext batch of config 3 (303 MB); packing into pvw_host_alloc memory
against the D2H copy of the words; pvw_load_pk_wire against pvw_load_pk from host words (wall clock).

    python tools/wire_timing.py [--reps 20]
Prints one JSON object per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi  # noqa: E402
from pvw_rs_amd import workloads as W  # noqa: E402

VP = C.c_void_p


def call(p, name, *args):
    rc = getattr(p._lib, name)(p._h, *args)
    if rc:
        raise P.PvwError(rc, _ffi.last_error(p._lib))


STREAM = None                      # a stream of our own: the legacy default stream's handle (0) would mean the context's stream


def timed(fn, reps, warm=3):
    s = STREAM
    for _ in range(warm):
        fn(s)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record(s)
        for _ in range(reps):
            fn(s)
        b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / reps


def codec(p, count, label, reps):
    Pw = p.L * p.l
    pb = p.wire_poly_bytes()
    q = torch.tensor(p.moduli(), dtype=torch.int64, device="cuda")
    d = torch.randint(0, 1 << 62, (count, p.L, p.l), dtype=torch.int64, device="cuda") % q.view(1, -1, 1)
    out = torch.empty(count * pb + 16, dtype=torch.uint8, device="cuda")
    back = torch.empty(count * Pw, dtype=torch.int64, device="cuda")
    bad = torch.zeros(2, dtype=torch.int64, device="cuda")
    words, packed = count * Pw * 8, count * pb
    ms = timed(lambda s: call(p, "pvw_wire_pack_device", VP(d.data_ptr()), count, VP(out.data_ptr()), VP(s.cuda_stream)), reps)
    print(json.dumps({"what": "wire_pack_kernel", "object": label, "polys": count, "word_bytes": words, "packed_bytes": packed,
                      "ms": round(ms, 4), "GBps_read_plus_written": round((words + packed) / ms / 1e6, 1)}))
    ms = timed(lambda s: call(p, "pvw_wire_unpack_device", VP(out.data_ptr()), count, VP(back.data_ptr()), VP(bad.data_ptr()),
                              VP(s.cuda_stream)), reps)
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and torch.equal(back.view_as(d), d)
    print(json.dumps({"what": "wire_unpack_kernel", "object": label, "polys": count, "ms": round(ms, 4),
                      "GBps_read_plus_written": round((words + packed) / ms / 1e6, 1)}))
    # into pvw_host_alloc memory vs the D2H copy of the words
    host = VP()
    assert p._lib.pvw_host_alloc(packed, C.byref(host)) == 0
    pinned = torch.empty(count * Pw, dtype=torch.int64, pin_memory=True)
    try:
        ms_h = timed(lambda s: call(p, "pvw_wire_pack_device", VP(d.data_ptr()), count, host, VP(s.cuda_stream)), max(2, reps // 4), 1)
        ms_c = timed(lambda s: pinned.copy_(d.view(-1), non_blocking=True), max(2, reps // 4), 1)
        torch.cuda.synchronize()
    finally:
        p._lib.pvw_host_free(host)
    print(json.dumps({"what": "pack_into_host_memory_vs_d2h_words", "object": label, "pack_to_host_ms": round(ms_h, 3),
                      "pack_to_host_GBps_of_packed": round(packed / ms_h / 1e6, 1), "d2h_words_ms": round(ms_c, 3),
                      "d2h_GBps": round(words / ms_c / 1e6, 1)}))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    global STREAM
    STREAM = torch.cuda.Stream()
    n, k, l, L = W.ENCRYPT_CONFIGS["c3"][:4]
    p = (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(W.bench_moduli(L)).build())
    d = codec(p, n * k, "config-3 public key", a.reps)
    del d
    torch.cuda.empty_cache()
    codec(p, 64 * (n + k), "64-dealer ciphertexts, config 3", a.reps)
    torch.cuda.empty_cache()
    # pvw_load_pk_wire vs pvw_load_pk from host words, pvw_get_pk_wire vs pvw_get_pk (synchronous host-buffer calls into
    # preallocated, touched host buffers; wall clock, best of 3)
    crs = P.PvwCrs.new_deterministic(p, bytes(32))
    gpk = P.GlobalPublicKey.new(crs)
    gpk.fill_uniform(bytes([1]) * 32)
    words = gpk.matrix(repr=P.REPR_NTT)
    body = np.ones(n * k * p.wire_poly_bytes(), dtype=np.uint8)
    wp, bp = VP(words.ctypes.data), VP(body.ctypes.data)
    call(p, "pvw_get_pk_wire", 0, n, bp, P.REPR_NTT)
    blob = body.nbytes
    res = {}
    for name, fn in (("load_pk_words", lambda: call(p, "pvw_load_pk", 0, n, wp, P.REPR_NTT)),
                     ("load_pk_wire", lambda: call(p, "pvw_load_pk_wire", 0, n, bp, P.REPR_NTT)),
                     ("get_pk_words", lambda: call(p, "pvw_get_pk", 0, n, wp, P.REPR_NTT)),
                     ("get_pk_wire", lambda: call(p, "pvw_get_pk_wire", 0, n, bp, P.REPR_NTT)),
                     ("python_to_bytes", lambda: gpk.to_bytes(repr=P.REPR_NTT))):
        fn()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        res[name + "_ms"] = round(min(t) * 1e3, 1)
    res.update(what="public-key load / get, config 3, host buffers", word_bytes=words.nbytes, packed_bytes=blob)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

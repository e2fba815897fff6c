"""python tools/encrypt_step_timing.py ROOT MODE [--tuning] [--config c3]
MODE steps: HIP events around 100 back-to-back seed-mode encrypts (5 repeats after 10 warm-up calls): us per step
MODE single: 200 isolated calls, events around each, a sync after every call: min / median / max us
then the host clock around call + sync on an idle stream.
Imports the package from ROOT (this tree, or a checkout of another commit built in place): profiles/r09_prologue_ahead_ab.txt."""
import ctypes as C
import json
import statistics
import sys

import torch

root, mode = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, workloads as W  # noqa: E402

if "--tuning" in sys.argv:
    _ffi.select("tuning")
cfg = sys.argv[sys.argv.index("--config") + 1] if "--config" in sys.argv else "c3"
n, k, l, L, _ = W.ENCRYPT_CONFIGS[cfg]
moduli = W.config_moduli(cfg, L)
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
p = (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).set_device(0)
     .set_secret_variance(W.SECRET_VARIANCE).set_error_bounds_u32(W.ERROR_BOUND_1, W.ERROR_BOUND_2).build())
crs = P.PvwCrs.new_deterministic(p, W.SEED_A)
gpk = P.GlobalPublicKey.new(crs)
gpk.fill_uniform(W.SEED_B)
lib = _ffi.lib()
scal = torch.tensor(W.scalars(n), dtype=torch.int64, device=dev)
c1 = torch.zeros((k, L, l), dtype=torch.int64, device=dev)
c2 = torch.zeros((n, L, l), dtype=torch.int64, device=dev)
rnd = _ffi.pvw_randomness_t()
rnd.mode = _ffi.RND_SEED
C.memmove(rnd.seed, W.SEED_ENC, 32)
s = torch.cuda.Stream(device=dev)
cs = C.c_void_p(s.cuda_stream)


def step():
    rc = lib.pvw_encrypt_device(p._h, C.c_void_p(scal.data_ptr()), n, C.byref(rnd), C.c_void_p(c1.data_ptr()),
                                C.c_void_p(c2.data_ptr()), P.REPR_NTT, cs)
    assert rc == 0, _ffi.last_error()


for _ in range(10):
    step()
torch.cuda.synchronize()
out = {"root": root, "mode": mode, "config": cfg, "tuning": "--tuning" in sys.argv}
if mode == "steps":
    reps = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(s)
        for _ in range(100):
            step()
        b.record(s)
        torch.cuda.synchronize()
        reps.append(a.elapsed_time(b) * 10.0)      # ms / 100 steps -> us per step
    out["us_per_step"] = [round(x, 2) for x in reps]
else:
    ts = []
    for _ in range(200):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        step()
        b.record(s)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    out["single_call_us"] = {"min": round(min(ts), 2), "median": round(statistics.median(ts), 2), "max": round(max(ts), 2)}
    import time
    hs = []
    for _ in range(200):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        s.synchronize()
        hs.append((time.perf_counter() - t0) * 1e6)
    out["single_call_host_us"] = {"min": round(min(hs), 2), "median": round(statistics.median(hs), 2), "max": round(max(hs), 2)}
print(json.dumps(out), flush=True)

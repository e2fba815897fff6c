"""The launch sequence of the twelve encrypt entry points ({pvw_encrypt, pvw_encrypt_multi, pvw_deal_shares} x {seeds, _rs} x
{host buffers, _device}): with pvw_ctx_set_profiling on, the per-name launch counts of pvw_ctx_kernel_time after one call,
against the table below, and for the _rs forms the counter advanced by exactly D.  n = 8, k = 32, l = 8 with one 56-bit modulus
(the 7-byte contraction), D = 1 (single forms), 2 (VALU), 3 (matrix-core threshold), 65 (one past PVW_MAX_PROLOGUE_KEYS) and
129 (one past a full GEMM pass of 16 * gemm_vb() dealers).  Power-basis output, so the inverse transforms count too.

The shipped library only: its dispatch thresholds are compiled in, the tuning build reads them from the environment per call.

A count is the number of times the library enqueued that step (one event pair each; the two inverse transforms of a call share
one), so the comparison is equality.  EXPECTED describes commit 18da36a, the last one before the encrypt half of the C API was
folded onto one key source and one entry frame.  It was worked out from that commit's encrypt_enqueue, encrypt_multi_enqueue and
shamir_enqueue (the rules are stated above the table); `python tests/_encrypt_launches_worker.py print` with that commit's
library prints the table in this form, and a run of it there has still to confirm these figures -- no GPU was to be had when
the table was written.  The seed and _rs twins and the host-buffer and device-pointer forms of one operation enqueue the same
steps, so the table is keyed by operation and D alone.

torch is imported FIRST so both libraries share one HIP runtime.  Spawned by tests/test_gpu_encrypt_launches.py; prints
LAUNCHES_OK."""
import ctypes as C
import os
import sys

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import EXAMPLE_MODULI  # noqa: E402

DEV = torch.device("cuda", 0)
SEED = bytes([0x2A]) * 32
S = bytes(range(101, 133))          # the randomness state's seed
NAMES = ("prologue", "mac_rows", "mac_rows_multi", "vec_digits", "gemm_digits", "shamir_eval", "intt")
N, K, L_RING = 8, 32, 8
DEGREE, PLAIN = 3, (1 << 31) - 1
DEALERS = (2, 3, 65, 129)

# (operation, D) -> launches in the order of NAMES, for commit 18da36a (see above): one prologue per 64 dealers of a pass, a pass
# of 4 dealers on the VALU (D < 3) or of 128 on the matrix cores, one shamir_eval scope per pass of a deal
EXPECTED = {
    ("single", 1): (1, 1, 0, 0, 0, 0, 1),
    ("multi", 2): (1, 0, 1, 0, 0, 0, 1),
    ("multi", 3): (1, 0, 0, 1, 1, 0, 1),
    ("multi", 65): (2, 0, 0, 1, 1, 0, 1),
    ("multi", 129): (3, 0, 0, 2, 2, 0, 1),
    ("deal", 2): (1, 0, 1, 0, 0, 1, 1),
    ("deal", 3): (1, 0, 0, 1, 1, 1, 1),
    ("deal", 65): (2, 0, 0, 1, 1, 1, 1),
    ("deal", 129): (3, 0, 0, 2, 2, 2, 1),
}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def seeds_for(D):
    return [bytes([(7 * d + i) & 0xFF for i in range(32)]) for d in range(D)]


def forms(p, gpk, st, s, D):
    """(operation, form name, is _rs, call) for every entry point that takes D dealers"""
    lib = _ffi.lib()
    cs = C.c_void_p(s.cuda_stream)
    scal = [[(1000 * d + i + 1) % (1 << 32) for i in range(N)] for d in range(D)]
    secrets = [(d * 7919 + 5) % PLAIN for d in range(D)]
    seeds = seeds_for(D)
    sd = np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()
    d_sc, d_se = dev(np.array(scal, dtype=np.uint64)), dev(np.array(secrets, dtype=np.uint64))
    c1 = torch.zeros((D, K, p.L, L_RING), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((D, N, p.L, L_RING), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    R = P.REPR_POWER
    chk = lambda rc: api._check(rc, lib)
    if D == 1:
        rnd, _ = api._randomness(p, seeds[0], None, None, None)
        return [
            ("single", "pvw_encrypt", False, lambda: P.encrypt(scal[0], gpk, seeds[0], repr=R)),
            ("single", "pvw_encrypt_rs", True, lambda: P.encrypt(scal[0], gpk, randomness=st, repr=R)),
            ("single", "pvw_encrypt_device", False,
             lambda: chk(lib.pvw_encrypt_device(p._h, ptr(d_sc), N, C.byref(rnd), ptr(c1), ptr(c2), R, cs))),
            ("single", "pvw_encrypt_rs_device", True,
             lambda: chk(lib.pvw_encrypt_rs_device(p._h, ptr(d_sc), N, st._h, ptr(c1), ptr(c2), R, cs))),
        ]
    return [
        ("multi", "pvw_encrypt_multi", False, lambda: P.encrypt_many(scal, gpk, seeds, R)),
        ("multi", "pvw_encrypt_multi_rs", True,
         lambda: p._call("pvw_encrypt_multi_rs", api._ptr(np.array(scal, dtype=np.uint64)), D, N, st._h,
                         api._ptr(np.zeros((D, K, p.L, L_RING), dtype=np.uint64)),
                         api._ptr(np.zeros((D, N, p.L, L_RING), dtype=np.uint64)), R)),
        ("multi", "pvw_encrypt_multi_device", False,
         lambda: chk(lib.pvw_encrypt_multi_device(p._h, ptr(d_sc), D, N, api._ptr(sd), ptr(c1), ptr(c2), R, cs))),
        ("multi", "pvw_encrypt_multi_rs_device", True,
         lambda: chk(lib.pvw_encrypt_multi_rs_device(p._h, ptr(d_sc), D, N, st._h, ptr(c1), ptr(c2), R, cs))),
        ("deal", "pvw_deal_shares", False, lambda: P.deal_party_shares(secrets, DEGREE, PLAIN, gpk, seeds=seeds, out_repr=R)),
        ("deal", "pvw_deal_shares_rs", True, lambda: P.deal_party_shares(secrets, DEGREE, PLAIN, gpk, randomness=st, out_repr=R)),
        ("deal", "pvw_deal_shares_device", False,
         lambda: chk(lib.pvw_deal_shares_device(p._h, ptr(d_se), D, DEGREE, PLAIN, api._ptr(sd), ptr(c1), ptr(c2), R, cs))),
        ("deal", "pvw_deal_shares_rs_device", True,
         lambda: chk(lib.pvw_deal_shares_rs_device(p._h, ptr(d_se), D, DEGREE, PLAIN, st._h, ptr(c1), ptr(c2), R, cs))),
    ]


def measure():
    """{(form name, operation, D): (launch counts, counter advance or None)} over all twelve entry points"""
    p = P.PvwParametersBuilder().set_parties(N).set_dimension(K).set_l(L_RING).set_moduli(EXAMPLE_MODULI[:1]).build()
    assert p._lib is _ffi.lib() and _ffi._selected == "default"      # the shipped library
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.fill_uniform(SEED)
    s = torch.cuda.Stream(device=DEV)
    got = {}
    with P.DeviceRandomness(p, S, 1000) as st:
        p.set_profiling(True)
        for D in (1,) + DEALERS:
            for op, name, is_rs, call in forms(p, gpk, st, s, D):
                before = st.counter(s)
                p.reset_profiling()
                call()
                s.synchronize()
                counts = tuple(p.kernel_time(nm)[1] for nm in NAMES)
                got[(name, op, D)] = (counts, st.counter(s) - before if is_rs else None)
        p.set_profiling(False)
    return got


def show(got):
    """the table as it goes into EXPECTED; the forms of one operation must agree for it to be keyed by (operation, D)"""
    table = {}
    for (name, op, D), (counts, _) in got.items():
        assert table.setdefault((op, D), counts) == counts, (name, D, counts, table[(op, D)])
    print("NAMES =", NAMES)
    for key in sorted(table, key=lambda x: (("single", "multi", "deal").index(x[0]), x[1])):
        print(f"    {key!r}: {table[key]!r},")


def check(got):
    assert len({name for name, _, _ in got}) == 12 and len(got) == 4 + 8 * len(DEALERS)
    for (name, op, D), (counts, advance) in got.items():
        print(name, D, dict(zip(NAMES, counts)), advance, flush=True)
        assert counts == EXPECTED[(op, D)], (name, D, dict(zip(NAMES, counts)), dict(zip(NAMES, EXPECTED[(op, D)])))
        assert advance in (None, D), (name, D, advance)
        assert (advance is None) == ("_rs" not in name), name


if __name__ == "__main__":
    assert torch.cuda.is_available()
    result = measure()
    if sys.argv[1:] == ["print"]:
        show(result)
    else:
        check(result)
        print("LAUNCHES_OK")

"""Encrypt from a device randomness state (pvw_rnd_state, pvw_encrypt_rs*, pvw_encrypt_multi_rs*) with torch tensors as
device memory and torch streams.  torch is imported FIRST so both libraries share one HIP runtime.  Spawned by
tests/test_gpu_device_randomness.py: `python _device_rnd_worker.py <case>` prints RND_OK on success."""
import ctypes as C
import os
import sys

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi  # noqa: E402
from _util import EXAMPLE_MODULI  # noqa: E402

S = bytes(range(101, 133))          # the state's seed
DEV = torch.device("cuda", 0)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def scalars(n, salt):
    return [(salt * 1000003 + 7919 * j + (j << 33)) % (1 << 64) for j in range(n)]


def dev_scalars(vals):
    return torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to(DEV)


def cseed(c):
    return P.DeviceRandomness.call_seed(S, c)


def _params(n, k, l, moduli, shard=None):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if shard:
        b = b.set_shard(*shard)
    return b.build()


def eager_single():
    """pvw_encrypt_rs_device three times in a row on one stream (no host wait between): bit-equal to the seed-mode encrypt
    under call_seed(S, c), c+1, c+2 (across the 2^32 boundary of the counter); the counter then reads c+3.  At config 3 and on
    a ragged party / CRS-row shard.  Then the host-buffer pvw_encrypt_rs, the fourth draw."""
    lib = _ffi.lib()
    for (n, k, l, L, shard) in [(4096, 256, 8, 17, None), (70, 128, 8, 3, (13, 51, 16, 83))]:
        p = _params(n, k, l, M.bench_moduli(L), shard)
        gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, S))
        gpk.fill_uniform(S)
        rA, rB = p.c1_hi - p.c1_lo, p.party_hi - p.party_lo
        c0 = (1 << 32) - 2
        s = torch.cuda.Stream(device=DEV)
        with P.DeviceRandomness(p, S, c0) as st:
            outs = []
            vals = [scalars(n, i) for i in range(3)]
            with torch.cuda.stream(s):
                for i in range(3):
                    sc = dev_scalars(vals[i])
                    c1 = torch.zeros((rA, L, l), dtype=torch.int64, device=DEV)
                    c2 = torch.zeros((rB, L, l), dtype=torch.int64, device=DEV)
                    P.api._check(lib.pvw_encrypt_rs_device(p._h, ptr(sc), n, st._h, ptr(c1), ptr(c2), P.REPR_NTT,
                                                           C.c_void_p(s.cuda_stream)))
                    outs.append((sc, c1, c2))
            assert st.counter(s) == c0 + 3, st.counter(s)
            for i in range(3):
                want = P.encrypt(vals[i], gpk, cseed(c0 + i))
                assert np.array_equal(u64(outs[i][1]), want.c1[p.c1_lo:p.c1_hi]), f"n={n} call {i}: c1"
                assert np.array_equal(u64(outs[i][2]), want.c2[p.party_lo:p.party_hi]), f"n={n} call {i}: c2"
            assert not np.array_equal(u64(outs[0][1]), u64(outs[1][1]))
            # the host-buffer entry point continues the sequence
            v3 = scalars(n, 3)
            got = P.encrypt(v3, gpk, randomness=st, repr=P.REPR_POWER)
            want = P.encrypt(v3, gpk, cseed(c0 + 3), repr=P.REPR_POWER)
            assert np.array_equal(got.c1, want.c1) and np.array_equal(got.c2, want.c2), f"n={n}: pvw_encrypt_rs"
            assert st.counter() == c0 + 4
            # set_counter is stream-ordered; the next draw starts there
            st.set_counter(5, s)
            assert st.counter(s) == 5
        print(f"eager single n={n} ok")


def graph_single():
    """pvw_prepare, then pvw_encrypt_rs_device captured into a graph (the shape of _device_api_worker.graph_capture) and
    replayed three times with new scalars: replay i equals the seed-mode encrypt under call_seed(S, c+i), c1 differs between
    every pair of replays, the counter then reads c+3, and the parties decrypt each replay's scalars."""
    lib = _ffi.lib()
    n, k, l, L = 70, 256, 8, 3
    p = _params(n, k, l, M.bench_moduli(L))
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, S))
    parties = [P.Party.new(i, p, S) for i in range(n)]
    gpk.generate_all_party_keys(parties, S)
    s = torch.cuda.Stream(device=DEV)
    assert p.prepare(P.PREPARE_PACKED, s.cuda_stream) > 0 and p.packed_active() == 61
    c0 = 1000
    st = P.DeviceRandomness(p, S, c0)
    scal = torch.zeros(n, dtype=torch.int64, device=DEV)
    c1 = torch.zeros((k, L, l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((n, L, l), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = lib.pvw_encrypt_rs_device(p._h, ptr(scal), n, st._h, ptr(c1), ptr(c2), P.REPR_NTT,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    P.api._check(rc)
    c1s = []
    for rep in range(3):
        vals = [(rep * 1000003 + 17 * j) % (1 << 32) for j in range(n)]
        scal.copy_(torch.tensor(vals, dtype=torch.int64))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = P.encrypt(vals, gpk, cseed(c0 + rep))
        got1, got2 = u64(c1), u64(c2)
        assert np.array_equal(got1, want.c1), f"graph replay {rep}: c1"
        assert np.array_equal(got2, want.c2), f"graph replay {rep}: c2"
        ct = P.PvwCiphertext(got1.copy(), got2.copy(), p, P.REPR_NTT)
        for i in (0, 1, 37, n - 1):
            assert P.decrypt_party_value(ct, parties[i].secret_key, i) == vals[i], f"replay {rep}: party {i}"
        c1s.append(got1.copy())
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.array_equal(c1s[a], c1s[b]), f"replays {a} and {b} share r"
    assert st.counter(s) == c0 + 3
    del g
    st.free()
    print("graph single ok")


def _multi_device(lib, p, st, vals, s):
    D, n = len(vals), p.n
    sc = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to(DEV)
    c1 = torch.zeros((D, p.k, p.L, p.l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((D, n, p.L, p.l), dtype=torch.int64, device=DEV)
    P.api._check(lib.pvw_encrypt_multi_rs_device(p._h, ptr(sc), D, n, st._h, ptr(c1), ptr(c2), P.REPR_NTT,
                                                 C.c_void_p(s.cuda_stream)))
    return sc, c1, c2


def multi():
    """pvw_encrypt_multi_rs_device at D = 2 (VALU), 3, 64, 130 (matrix cores; 130 = two dealer groups, the first of two
    64-key prologue windows), 7- and 8-byte moduli: bit-equal to pvw_encrypt_multi with seeds[d] = call_seed(S, c+d), the
    counter advancing by D; the host-buffer pvw_encrypt_multi_rs through encrypt_all_party_shares; then one multi-dealer
    encrypt captured after pvw_prepare(PVW_PREPARE_MFMA) and replayed twice: fresh and correct each time."""
    lib = _ffi.lib()
    n, k, l = 40, 64, 8
    for moduli in (EXAMPLE_MODULI[:2], M.bench_moduli(2)):
        p = _params(n, k, l, moduli)
        gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, S))
        gpk.fill_uniform(S)
        s = torch.cuda.Stream(device=DEV)
        c = 77
        with P.DeviceRandomness(p, S, c) as st:
            for D in (2, 3, 64, 130):
                vals = [scalars(n, 10 * D + d) for d in range(D)]
                _, c1, c2 = _multi_device(lib, p, st, vals, s)
                assert st.counter(s) == c + D, (D, st.counter(s))
                want = P.encrypt_many(vals, gpk, [cseed(c + d) for d in range(D)])
                g1, g2 = u64(c1), u64(c2)
                for d in range(D):
                    assert np.array_equal(g1[d], want[d].c1), f"q={moduli[0]:#x} D={D} dealer {d}: c1"
                    assert np.array_equal(g2[d], want[d].c2), f"q={moduli[0]:#x} D={D} dealer {d}: c2"
                c += D
            shares = [scalars(n, 900 + d) for d in range(n)]
            got = P.encrypt_all_party_shares(shares, gpk, randomness=st)
            want = P.encrypt_many(shares, gpk, [cseed(c + d) for d in range(n)])
            assert all(np.array_equal(a.c1, b.c1) and np.array_equal(a.c2, b.c2) for a, b in zip(got, want)), "multi host"
            c += n
            assert st.counter() == c
            # captured after pvw_prepare(PVW_PREPARE_MFMA), replayed twice
            D = 64
            p.prepare(P.PREPARE_MFMA, s.cuda_stream)
            sc = torch.zeros((D, n), dtype=torch.int64, device=DEV)
            c1 = torch.zeros((D, k, p.L, l), dtype=torch.int64, device=DEV)
            c2 = torch.zeros((D, n, p.L, l), dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = lib.pvw_encrypt_multi_rs_device(p._h, ptr(sc), D, n, st._h, ptr(c1), ptr(c2), P.REPR_NTT,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
            P.api._check(rc)
            first = None
            for rep in range(2):
                vals = [scalars(n, 5000 + 100 * rep + d) for d in range(D)]
                sc.copy_(torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)))
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                want = P.encrypt_many(vals, gpk, [cseed(c + D * rep + d) for d in range(D)])
                g1, g2 = u64(c1), u64(c2)
                for d in range(D):
                    assert np.array_equal(g1[d], want[d].c1) and np.array_equal(g2[d], want[d].c2), f"replay {rep} dealer {d}"
                if first is None:
                    first = g1.copy()
                else:
                    assert not any(np.array_equal(first[d], g1[d]) for d in range(D)), "replays share r"
            assert st.counter(s) == c + 2 * D
            del g
        print(f"multi q={moduli[0]:#x} ok")


def capture_unprepared():
    """A multi-dealer encrypt on the matrix cores captured without pvw_prepare(PVW_PREPARE_MFMA): InvalidParameters naming
    pvw_prepare, for the seed and the state entry point alike, and the capture still ends without error."""
    lib = _ffi.lib()
    n, k, l, L, D = 40, 64, 8, 2, 8
    p = _params(n, k, l, M.bench_moduli(L))
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, S))
    gpk.fill_uniform(S)
    st = P.DeviceRandomness(p, S, 0)
    sc = torch.zeros((D, n), dtype=torch.int64, device=DEV)
    c1 = torch.zeros((D, k, L, l), dtype=torch.int64, device=DEV)
    c2 = torch.zeros((D, n, L, l), dtype=torch.int64, device=DEV)
    seeds = np.frombuffer(S * D, dtype=np.uint8).copy()
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc1 = lib.pvw_encrypt_multi_rs_device(p._h, ptr(sc), D, n, st._h, ptr(c1), ptr(c2), P.REPR_NTT, cs)
        msg1 = _ffi.last_error(lib)
        rc2 = lib.pvw_encrypt_multi_device(p._h, ptr(sc), D, n, seeds.ctypes.data_as(C.c_void_p), ptr(c1), ptr(c2),
                                           P.REPR_NTT, cs)
        msg2 = _ffi.last_error(lib)
    torch.cuda.synchronize()
    assert rc1 == 1 and "pvw_prepare" in msg1, (rc1, msg1)
    assert rc2 == 1 and "pvw_prepare" in msg2, (rc2, msg2)
    del g                                        # nothing was captured
    assert st.counter() == 0
    # eager calls are unaffected
    vals = [scalars(n, d) for d in range(D)]
    _, c1, c2 = _multi_device(lib, p, st, vals, s)
    want = P.encrypt_many(vals, gpk, [cseed(d) for d in range(D)])
    assert all(np.array_equal(u64(c2)[d], want[d].c2) for d in range(D))
    assert st.counter(s) == D
    st.free()
    print("capture unprepared ok")


def free_clears():
    """pvw_rnd_state_free clears the device seed before it releases the memory"""
    n, k, l, L = 16, 32, 8, 2
    p = _params(n, k, l, M.bench_moduli(L))
    st = P.DeviceRandomness(p, S, 3)
    assert st.counter() == 3
    st.free()
    assert P.api._rnd_free_residue(p._lib) == 0
    st.free()                                    # a second free is a no-op
    print("free ok")


CASES = {f.__name__: f for f in (eager_single, graph_single, multi, capture_unprepared, free_clears)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("RND_OK")

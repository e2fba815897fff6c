"""Sums of dealers' ciphertexts on the device against pvw_ct_sum_host and the per-dealer decrypts.  torch is
imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_ct_sum.py; prints CT_SUM_OK."""
import ctypes as C
import os
import sys

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import EXAMPLE_MODULI  # noqa: E402
from test_ct_sum_host import GEOMETRIES, _params, _words  # noqa: E402

DEV = torch.device("cuda", 0)
U64 = (1 << 64) - 1
SEED = bytes([0x2A]) * 32


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def host_sum(p, c1s, c2s, valid, lo, hi):
    c1, c2 = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((hi - lo, p.L, p.l), np.uint64)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    p._call("pvw_ct_sum_host", api._ptr(c1s), api._ptr(c2s), len(c1s), api._ptr(v), lo, hi, api._ptr(c1), api._ptr(c2), None)
    return c1, c2


def device_sum(p, d_c1s, d_c2s, D, valid, lo, hi, stream):
    """pvw_ct_sum_device on `stream`: (c1, c2, count)"""
    c1 = torch.full((p.k, p.L, p.l), -1, dtype=torch.int64, device=DEV)
    c2 = torch.full((hi - lo, p.L, p.l), -1, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    v = None if valid is None else dev(np.ascontiguousarray(valid, dtype=np.uint8))
    torch.cuda.synchronize()
    p._call("pvw_ct_sum_device", ptr(d_c1s), ptr(d_c2s), D, ptr(v), lo, hi, ptr(c1), ptr(c2), ptr(cnt), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return u64(c1), u64(c2), int(cnt.item())


def sums():
    """the host-test matrix: every geometry, D in {1, 2, 7, 130}, reduced / any / extreme words, masks (all, alternating, one
    dealer, none), row ranges, on a caller's own stream, in the shipped library and in every kernel form of the tuning build"""
    s = torch.cuda.Stream(device=DEV)
    for which, splits in (("default", [0]), ("tuning", [1, 3, 64])):
        _ffi.select(which)
        for split in splits:
            os.environ["PVW_SUM_SPLIT"] = str(split)
            for geom, (n, k, l, moduli) in enumerate(GEOMETRIES):
                p = _params(n, k, l, moduli)
                for D in (1, 2, 7, 130):
                    rng = np.random.default_rng(1000 * geom + D)
                    masks = [None, np.arange(D) % 2 == 0, np.arange(D) == D // 2, np.zeros(D, bool)]
                    ranges = [(0, n), (1, n), (n - 1, n), (0, 1)]
                    for i, kind in enumerate(["reduced", "any", "extreme"]):
                        c1s, c2s = _words(rng, p, D, k, kind), _words(rng, p, D, n, kind)
                        d1, d2 = dev(c1s), dev(c2s)
                        for j, valid in enumerate(masks):
                            lo, hi = ranges[(i + j) % len(ranges)]
                            g1, g2, cnt = device_sum(p, d1, d2, D, valid, lo, hi, s)
                            what = (which, split, geom, D, kind, j, lo, hi)
                            if valid is not None and not valid.any():       # the device form sums nothing: zeros, count 0
                                assert not g1.any() and not g2.any() and cnt == 0, what
                                continue
                            w1, w2 = host_sum(p, c1s, c2s, valid, lo, hi)
                            assert np.array_equal(g1, w1) and np.array_equal(g2, w2), what
                            assert cnt == (D if valid is None else int(np.count_nonzero(valid))), what
                            if which == "default" and kind != "reduced":
                                h1, h2, hc = np.zeros_like(w1), np.zeros_like(w2), C.c_uint32()
                                v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
                                p._call("pvw_ct_sum", api._ptr(c1s), api._ptr(c2s), D, api._ptr(v), lo, hi, api._ptr(h1), api._ptr(h2),
                                        C.byref(hc))
                                assert np.array_equal(h1, w1) and np.array_equal(h2, w2) and hc.value == cnt, what
            print(f"sums {which} split={split} ok", flush=True)
    os.environ.pop("PVW_SUM_SPLIT")
    _ffi.select("default")


def _big(name, n, k, l, moduli, D, lo, hi, s, valid=None):
    p = _params(n, k, l, moduli)
    g = torch.Generator(device=DEV)
    g.manual_seed(D + n)
    d1 = torch.empty((D, k, p.L, l), dtype=torch.int64, device=DEV).random_(generator=g)
    d2 = torch.empty((D, n, p.L, l), dtype=torch.int64, device=DEV).random_(generator=g)
    for t in (d1, d2):                                           # random_ leaves bit 63 clear
        t.bitwise_xor_(t.bitwise_left_shift(13))
    w1, w2 = host_sum(p, u64(d1), u64(d2), valid, lo, hi)
    g1, g2, cnt = device_sum(p, d1, d2, D, valid, lo, hi, s)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2), name
    assert cnt == (D if valid is None else int(np.count_nonzero(valid))), name
    print(f"{name} ok", flush=True)
    return p, d1, d2, w1, w2


def big():
    """the production geometries, any 64-bit words.  Config 3 (k = 256, l = 8, 17 moduli): D = 1024 over 256 parties and
    D = 128 over all 4096 (the [D][n] buffer of 1024 x 4096 rows is 4.5 GB; the kernel sees the same strides either way).
    Config-5 shard (k = 512, l = 16, 34 moduli): D = 1024, whole rows and, through pvw_decrypt_sum_*, the column form: the
    noisy polynomial of the device sum equals the single decrypt of the host-summed ciphertext."""
    s = torch.cuda.Stream(device=DEV)
    m17, m34 = M.bench_moduli(17), M.bench_moduli(34)
    half = np.arange(1024) % 2 == 1
    _big("config 3, D=1024, 256 parties, rows [0, 256)", 256, 256, 8, m17, 1024, 0, 256, s)
    _big("config 3, D=1024, masked, rows [3, 200)", 256, 256, 8, m17, 1024, 3, 200, s, half)
    _big("config 3, D=128, rows [0, 4096)", 4096, 256, 8, m17, 128, 0, 4096, s)
    p, d1, d2, w1, w2 = _big("config-5 shard, D=1024, rows [0, 2)", 2, 512, 16, m34, 1024, 0, 2, s, half)
    # column form: party 1's column, the resident key, the noisy polynomial as an output
    rng = np.random.default_rng(11)
    sk = rng.integers(-1, 2, (p.k, p.l), dtype=np.int64)
    col = d2[:, 1].contiguous()
    outs = [torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(2)]
    st, cnt = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    nz = torch.zeros((p.L, p.l), dtype=torch.int64, device=DEV)
    d_half, d_sk, d_w1, d_w2 = dev(half.astype(np.uint8)), dev(sk), dev(w1[None]), dev(w2[1][None])
    ref_nz = torch.zeros((1, p.L, p.l), dtype=torch.int64, device=DEV)
    with P.DeviceSecretKey(P.SecretKey(p, sk)) as key:
        torch.cuda.synchronize()
        key.decrypt_sum_device_checked(d1, col, 1024, outs[0], d_valid=d_half, d_noisy=nz, d_noise=outs[1], d_status=st, d_count=cnt,
                                       stream=s)
        s.synchronize()
        p._call("pvw_decrypt_noisy_device", ptr(d_sk), ptr(d_w1), ptr(d_w2), 1, P.REPR_NTT, ptr(ref_nz), C.c_void_p(s.cuda_stream))
        s.synchronize()
    print("column form: count", int(cnt.item()), "noisy equal", bool(np.array_equal(u64(nz), u64(ref_nz)[0])), flush=True)
    assert np.array_equal(u64(nz), u64(ref_nz)[0]) and int(cnt.item()) == 512, "column form"
    ref = P.decode_scalar_pvw_checked_host(p, u64(ref_nz))
    assert (int(u64(outs[0])[0]), int(u64(outs[1])[0]), int(st.item())) == (int(ref.values[0]), int(ref.noise[0]), int(ref.status[0]))
    assert api._secret_residue(p)[0] == 0
    print("config-5 shard column form ok", flush=True)


def system(moduli, n, k, l):
    p = _params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


def triple(r, i=0):
    return int(r.values[i]), int(r.noise[i]), int(r.status[i])


def decrypt():
    """dealt ciphertexts (pvw_keygen + pvw_encrypt_multi), D = 64 <= capacity: every sum entry point returns the sum of the
    per-dealer decrypts and the report of pvw_decode_checked_host on the noisy polynomial of the host-summed ciphertext"""
    n, k, l, D = 24, 32, 8, 64
    for name, moduli in (("5x61", M.bench_moduli(5)), ("4x56", EXAMPLE_MODULI)):
        p, gpk, parties = system(moduli, n, k, l)
        assert p.sum_capacity() >= D, name
        rng = np.random.default_rng(7)
        shares = rng.integers(0, 1 << 57, (D, n), dtype=np.uint64)
        cts = P.encrypt_many(shares.tolist(), gpk, [api._dealer_seed(SEED, d) for d in range(D)])
        valid = np.arange(D) % 3 != 1
        for v in (None, valid):
            on = [d for d in range(D) if v is None or v[d]]
            agg = P.aggregate_ciphertexts(cts, v)
            h1, h2 = host_sum(p, np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts]), v, 0, n)
            assert np.array_equal(agg.c1, h1) and np.array_equal(agg.c2, h2) and agg.repr == cts[0].repr, name
            back = P.PvwCiphertext.from_bytes(p, agg.to_bytes())
            assert np.array_equal(back.c1, agg.c1) and np.array_equal(back.c2, agg.c2), name
            want = [sum(int(shares[d][i]) for d in on) for i in range(n)]
            refs = []
            for i in range(n):
                _, noisy = api._decrypt_batch(p, [agg], parties[i].secret_key, i, True)
                refs.append(P.decode_scalar_pvw_checked_host(p, noisy))
                assert triple(refs[i])[0] == want[i] and not refs[i].lossy[0], (name, i)
            for i in (0, 5, n - 1):
                r = P.decrypt_party_sum(cts, parties[i].secret_key, i, v)
                assert triple(r) == triple(refs[i]) and r.valid[0] and r.bound == len(on) * p.noise_bound(), (name, i)
                vals = api._decrypt_batch_checked(p, [cts[d] for d in on], parties[i].secret_key, i, p.noise_bound())
                assert sum(int(x) for x in vals.values) == want[i] and not vals.lossy.any(), (name, i)
                assert int(r.noise[0]) <= sum(int(x) for x in vals.noise), (name, i)
                assert api._secret_residue(p)[0] == 0, name
            # POWER-basis copies for the device form (made before the keyed calls: a transform reuses the pooled staging)
            c1 = dev(np.stack([p.ntt_inverse(c.c1) for c in cts]))
            c2 = dev(np.stack([p.ntt_inverse(c.c2) for c in cts]))
            for lo, cnt in ((1, 5), (0, n)):                       # both sides of the 22-party dispatch
                r = P.decrypt_all_party_sums(cts, parties[lo:lo + cnt], v)
                assert [triple(r, j) for j in range(cnt)] == [triple(refs[lo + j]) for j in range(cnt)], (name, lo, cnt)
                assert api._secret_residue(p)[0] == 0, name
                # device pointers, POWER basis in (the sum is transformed in scratch)
                sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties[lo:lo + cnt]]).astype(np.int64))
                out, nz = torch.zeros(cnt, dtype=torch.int64, device=DEV), torch.zeros(cnt, dtype=torch.int64, device=DEV)
                st, dc = torch.zeros(cnt, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
                dv = None if v is None else dev(v.astype(np.uint8))
                torch.cuda.synchronize()
                p._call("pvw_decrypt_all_sum_checked_device", lo, lo + cnt, ptr(sk), ptr(c1), ptr(c2), D, ptr(dv), P.REPR_POWER, ptr(out),
                        ptr(nz), ptr(st), ptr(dc), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                torch.cuda.synchronize()
                got = list(zip(u64(out).tolist(), u64(nz).tolist(), st.cpu().tolist()))
                assert got == [triple(refs[lo + j]) for j in range(cnt)] and int(dc.item()) == len(on), (name, lo, cnt)
                assert api._secret_residue(p)[0] == 0, name
        # the device form with coefficients and with the resident key, NTT basis in
        i = 4
        c1, c2col = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2[i] for c in cts]))
        dv = dev(valid.astype(np.uint8))
        for resident in (False, True):
            out, nz = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
            st, dc = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            stream = torch.cuda.current_stream()
            torch.cuda.synchronize()
            if resident:
                with P.DeviceSecretKey(parties[i].secret_key) as key:
                    key.decrypt_sum_device_checked(c1, c2col, D, out, d_valid=dv, d_noise=nz, d_status=st, d_count=dc, stream=stream)
                    torch.cuda.synchronize()
            else:
                sk = dev(parties[i].secret_key.secret_coeffs.astype(np.int64))
                p._call("pvw_decrypt_sum_checked_device", ptr(sk), ptr(c1), ptr(c2col), D, ptr(dv), P.REPR_NTT, None, ptr(out), ptr(nz),
                        ptr(st), ptr(dc), C.c_void_p(stream.cuda_stream))
                torch.cuda.synchronize()
            want = P.decrypt_party_sum(cts, parties[i].secret_key, i, valid)
            assert (int(u64(out)[0]), int(u64(nz)[0]), int(st.item())) == triple(want) and int(dc.item()) == int(valid.sum()), (name, resident)
            assert api._secret_residue(p)[0] == 0, name
        # shares near 2^63: the sum of the plaintexts is not representable
        big = np.full((3, n), (1 << 63) - 9, dtype=np.uint64)
        bcts = P.encrypt_many(big.tolist(), gpk, [api._dealer_seed(SEED, 900 + d) for d in range(3)])
        r = P.decrypt_party_sum(bcts, parties[2].secret_key, 2)
        assert r.lossy[0] and not r.valid[0] and int(r.noise[0]) <= 3 * p.noise_bound(), name
        assert P.decrypt_all_party_sums(bcts, parties).lossy.all(), name
        # a wrong key, a tampered c2: the noise saturates
        r = P.decrypt_party_sum(cts, parties[3].secret_key, 2)
        assert int(r.noise[0]) == U64 and not r.valid[0], name
        bad = [P.PvwCiphertext(c.c1.copy(), c.c2.copy(), p, c.repr) for c in cts]
        e = np.zeros((p.L, p.l), dtype=np.uint64)
        e[:, 1] = [(1 << 70) % q for q in p.moduli()]
        q = np.array(p.moduli(), dtype=object)[:, None]
        bad[5].c2[2] = ((bad[5].c2[2].astype(object) + p.ntt_forward(e).astype(object)) % q).astype(np.uint64)
        r = P.decrypt_party_sum(bad, parties[2].secret_key, 2)
        assert int(r.noise[0]) == U64 and not r.valid[0], name
        assert api._secret_residue(p)[0] == 0, name
        print(f"decrypt {name} ok", flush=True)


def capture():
    """after pvw_prepare(PVW_PREPARE_SUM) a captured pvw_ct_sum_device + pvw_decrypt_sum_device_sk_checked replays with a changed
    mask and gives the new sum; without it the captured calls return the error and the capture survives"""
    lib = _ffi.lib()
    n, k, l, D = 6, 32, 8, 40
    p, gpk, parties = system(M.bench_moduli(5), n, k, l)
    rng = np.random.default_rng(3)
    shares = rng.integers(0, 1 << 57, (D, n), dtype=np.uint64)
    cts = P.encrypt_many(shares.tolist(), gpk, [api._dealer_seed(SEED, d) for d in range(D)])
    i = 3
    c1, c2 = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2 for c in cts]))
    col = c2[:, i].contiguous()
    mask = torch.ones(D, dtype=torch.uint8, device=DEV)
    o1 = torch.zeros((k, p.L, l), dtype=torch.int64, device=DEV)
    o2 = torch.zeros((n, p.L, l), dtype=torch.int64, device=DEV)
    out, nz = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    st, dc = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    with P.DeviceSecretKey(parties[i].secret_key) as key:
        def enqueue(cs):
            rc1 = lib.pvw_ct_sum_device(p._h, ptr(c1), ptr(c2), D, ptr(mask), 0, n, ptr(o1), ptr(o2), ptr(dc), cs)
            m1 = _ffi.last_error(lib)
            rc2 = lib.pvw_decrypt_sum_device_sk_checked(p._h, key._h, ptr(c1), ptr(col), D, ptr(mask), P.REPR_NTT, None, ptr(out), ptr(nz),
                                                        ptr(st), C.c_void_p(dc.data_ptr() + 4), cs)
            return rc1, m1, rc2, _ffi.last_error(lib)
        # not prepared: a stream the context has never seen
        s0 = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s0):
            rc1, m1, rc2, m2 = enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc1 == 1 and "pvw_prepare" in m1 and rc2 == 1 and "pvw_prepare" in m2, (rc1, m1, rc2, m2)
        del g0
        # prepared
        s = torch.cuda.Stream(device=DEV)
        p.prepare(P.PREPARE_SUM, s.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc1, m1, rc2, m2 = enqueue(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc1 == 0 and rc2 == 0, (m1, m2)
        for rep, v in enumerate((np.ones(D, bool), np.arange(D) % 2 == 0, np.arange(D) == 7)):
            mask.copy_(torch.from_numpy(v.astype(np.uint8)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            w1, w2 = host_sum(p, np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts]), v, 0, n)
            assert np.array_equal(u64(o1), w1) and np.array_equal(u64(o2), w2), rep
            want = P.decrypt_party_sum(cts, parties[i].secret_key, i, v)
            assert (int(u64(out)[0]), int(u64(nz)[0]), int(st.item())) == triple(want), rep
            assert int(u64(out)[0]) == sum(int(shares[d][i]) for d in range(D) if v[d]), rep
            assert dc.cpu().tolist() == [int(v.sum())] * 2, rep
        del g
    assert api._secret_residue(p)[0] == 0
    print("capture ok", flush=True)


def shard():
    """a sharded context sums its rows to the same words as the unsharded one"""
    n, k, l, D = 12, 8, 16, 9
    moduli = M.bench_moduli(3)
    full = _params(n, k, l, moduli)
    part = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).set_shard(4, 9, 2, 6).build()
    rng = np.random.default_rng(2)
    c1s, c2s = _words(rng, full, D, k, "any"), _words(rng, full, D, n, "any")
    valid = np.arange(D) % 4 != 2
    s = torch.cuda.Stream(device=DEV)
    a1, a2, ac = device_sum(full, dev(c1s), dev(c2s), D, valid, 0, n, s)
    b1, b2, bc = device_sum(part, dev(c1s), dev(c2s), D, valid, 4, 9, s)
    assert np.array_equal(a1, b1) and np.array_equal(a2[4:9], b2) and ac == bc == int(valid.sum())
    h1, h2 = np.zeros_like(b1), np.zeros_like(b2)
    part._call("pvw_ct_sum", api._ptr(c1s), api._ptr(c2s), D, api._ptr(valid.astype(np.uint8)), 4, 9, api._ptr(h1), api._ptr(h2), None)
    assert np.array_equal(h1, b1) and np.array_equal(h2, b2)
    print("shard ok", flush=True)


CASES = {f.__name__: f for f in (sums, big, decrypt, capture, shard)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("CT_SUM_OK")

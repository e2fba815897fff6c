"""The plain decode on the device against pvw_decode_plain_host and the per-dealer host sums, bit for bit.  torch
is imported FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_plain_decode.py; prints
PLAIN_DECODE_OK."""
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
import _plain_cases as PC  # noqa: E402
import test_checked_decode_host as TC  # noqa: E402

DEV = torch.device("cuda", 0)
U64 = (1 << 64) - 1
SEED = bytes([0x2A]) * 32
LOSSY, NEG, TRUNC = PC.DEC_LOSSY, PC.DEC_NEGATIVE, PC.DEC_WIDE_TRUNCATED


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """device buffers of one call: out / noise [shape], status [shape], wide [shape][ww], filled with a pattern first"""

    def __init__(self, shape, ww):
        shape = tuple(np.atleast_1d(shape))
        self.ww = ww
        self.out = torch.full(shape, -1, dtype=torch.int64, device=DEV)
        self.noise = torch.full(shape, -1, dtype=torch.int64, device=DEV)
        self.status = torch.full(shape, -1, dtype=torch.int32, device=DEV)
        self.wide = torch.full(shape + (ww,), -1, dtype=torch.int64, device=DEV) if ww else None
        self.count = torch.full((1,), -1, dtype=torch.int32, device=DEV)

    def rows(self):
        torch.cuda.synchronize()
        w = u64(self.wide) if self.ww else np.zeros(tuple(self.out.shape) + (0,), np.uint64)
        return u64(self.out), u64(self.noise), self.status.cpu().numpy().view(np.uint32), w


def same(tag, got, ref, ww):
    """got: (out, noise, status, wide) arrays; ref: a CheckedDecryption of pvw_decode_plain_host on the same polynomials"""
    out, noise, status, wide = got
    for what, a, b in (("out", out, ref.residues), ("noise", noise, ref.noise), ("status", status, ref.status)):
        a, b = np.ravel(a), np.ravel(b)
        assert a.shape == b.shape, (tag, what, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (tag, what, [(int(i), int(a[i]), int(b[i])) for i in bad[:4]])
    if ww:
        a, b = np.asarray(wide).reshape(-1, ww), wide_of(ref, ww)
        assert a.shape == b.shape and np.array_equal(a, b), (tag, "wide")


def decode():
    """both decode forms on the CPU test's inputs: the lifted chain (shipped library; tuning build with PVW_DECODE_SMALL=0:
    every lift in full) and the fixed-width form (tuning build, PVW_DECODE_VARIANT=1); host-buffer and device-pointer calls"""
    forms = (("default", {}), ("tuning", {"PVW_DECODE_SMALL": "0"}), ("tuning", {"PVW_DECODE_VARIANT": "1"}))
    for name in sorted(PC.SETS):
        moduli, l = PC.SETS[name]
        m = M.Params(3, 4, l, moduli)
        cases = PC.all_cases(m)
        noisy = PC.rns(cases, moduli)
        inputs = (("reduced", noisy), ("unreduced", PC.unreduce(noisy, moduli)))
        for which, env in forms:
            _ffi.select(which)
            os.environ.update(env)
            p = TC._params(moduli, l)
            for modulus, ww in PC.option_grid(m) + [(0, 0)]:
                for kind, nz in inputs:
                    ref = P.decode_scalar_pvw_plain_host(p, nz, modulus, ww)
                    if kind == "reduced":                # the host reference itself against the restated contract
                        w = PC.contract_arrays(cases, m, modulus, ww)
                        assert np.array_equal(ref.residues, w[0]) and np.array_equal(ref.noise, w[1]) and np.array_equal(ref.status, w[2])
                    r = P.decode_scalar_pvw_plain(p, nz, modulus, ww)
                    wd = np.array([[(abs(int(v)) >> (64 * w)) & U64 for w in range(ww)] for v in r.values], dtype=np.uint64)
                    same((name, which, env, modulus, ww, kind, "host buffers"), (r.residues, r.noise, r.status, wd), ref, ww)
                    o = Out(len(nz), ww)
                    d_nz = dev(nz)
                    torch.cuda.synchronize()
                    p._call("pvw_decode_plain_device", ptr(d_nz), len(nz), ptr(o.out), ptr(o.noise), ptr(o.status), modulus, ww,
                            ptr(o.wide), cur())
                    same((name, which, env, modulus, ww, kind, "device"), o.rows(), ref, ww)
                    assert np.array_equal(u64(d_nz), nz)                                   # power basis in: read only
            for key in env:
                os.environ.pop(key)
            print(f"decode {name} {which} {env} ok", flush=True)
    _ffi.select("default")


def system(moduli, n, k, l):
    p = TC._params(moduli, l, n=n, k=k)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


def deal(p, gpk, D, n, top, rng, base=0):
    shares = (rng.integers(0, 1 << 62, (D, n), dtype=np.uint64).astype(object) * (1 << 20) % top).astype(np.uint64)
    cts = P.encrypt_many(shares.tolist(), gpk, [api._dealer_seed(SEED, base + d) for d in range(D)])
    return shares, cts


def host_sum(p, cts, valid):
    c1, c2 = np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    c1s, c2s = np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts])
    p._call("pvw_ct_sum_host", api._ptr(c1s), api._ptr(c2s), len(cts), api._ptr(v), 0, p.n, api._ptr(c1), api._ptr(c2), None)
    return P.PvwCiphertext(c1, c2, p, cts[0].repr)


def refs_of(p, ct, parties, modulus, ww):
    """per party: pvw_decode_plain_host on the noisy polynomial of the single decrypt of `ct`"""
    nz = np.stack([api._decrypt_batch(p, [ct], parties[i].secret_key, i, True)[1][0] for i in range(len(parties))])
    return P.decode_scalar_pvw_plain_host(p, nz, modulus, ww), nz


def pick(ref, idx):
    class R:
        pass
    r = R()
    idx = np.atleast_1d(idx)
    r.values, r.residues, r.noise, r.status = ref.values[idx], ref.residues[idx], ref.noise[idx], ref.status[idx]
    return r


def wide_of(r, ww):
    return np.array([[(abs(int(v)) >> (64 * w)) & U64 for w in range(ww)] for v in np.ravel(r.values)], dtype=np.uint64)


def aggregate():
    """the case the feature exists for: n = k = 32, l = 8, 5 x 61-bit, D = 64 dealers dealing uniform shares below p = the first
    limb.  Every aggregate entry point: out == sum_d share mod p for every party, the wide words equal the integer sum,
    PVW_DEC_LOSSY is set -- and the checked call on the same buffers still returns its old word (0) and report"""
    n, k, l, D = 32, 32, 8, 64
    moduli = M.bench_moduli(5)
    p, gpk, parties = system(moduli, n, k, l)
    q0 = int(moduli[0])
    W = (p.q_total().bit_length() + 63) // 64
    assert p.sum_capacity() >= D
    rng = np.random.default_rng(8)
    shares, cts = deal(p, gpk, D, n, q0, rng)
    assert int(shares.max()) < q0 and int(shares.max()) > q0 // 2
    c1n, c2n = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2 for c in cts]))
    sk_all = np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64)
    for vi, v in enumerate((None, np.arange(D) % 3 != 1, np.arange(D) == 9)):
        on = [d for d in range(D) if v is None or v[d]]
        sums = [sum(int(shares[d][i]) for d in on) for i in range(n)]
        ref, nz = refs_of(p, host_sum(p, cts, v), parties, q0, W)
        assert [int(x) for x in ref.values] == sums and [int(x) for x in ref.residues] == [s % q0 for s in sums]
        if len(on) > 16:
            assert ((ref.status & LOSSY) != 0).all() and int(ref.noise.max()) <= len(on) * p.noise_bound()
        old = P.decrypt_all_party_sums(cts, parties, v)                       # the checked call: its old word and report
        assert np.array_equal(old.status, ref.status & np.uint32(LOSSY)) and np.array_equal(old.noise, ref.noise)
        assert all(int(old.values[i]) == (sums[i] if sums[i] <= U64 else 0) for i in range(n))
        dv = None if v is None else dev(v.astype(np.uint8))
        for lo, cnt in ((1, 5), (0, n)):                                     # both sides of the 22-party dispatch
            idx = np.arange(lo, lo + cnt)
            r = P.decrypt_all_party_sums(cts, parties[lo:lo + cnt], v, plain_modulus=q0, wide=True)
            same(("all_sum host", vi, lo), (r.residues, r.noise, r.status, wide_of(r, W)), pick(ref, idx), W)
            assert r.valid.all() and [int(x) for x in r.values] == sums[lo:lo + cnt]
            for modulus, ww in ((q0, W), (q0, 0), (0, 2), (2, 1)):
                sub = P.decode_scalar_pvw_plain_host(p, nz, modulus, ww)
                o = Out(cnt, ww)
                sk = dev(sk_all[lo:lo + cnt])
                torch.cuda.synchronize()
                p._call("pvw_decrypt_all_sum_plain_device", lo, lo + cnt, ptr(sk), ptr(c1n), ptr(c2n), D, ptr(dv), P.REPR_NTT, ptr(o.out),
                        ptr(o.noise), ptr(o.status), ptr(o.count), modulus, ww, ptr(o.wide), cur())
                same(("all_sum device", vi, lo, modulus, ww), o.rows(), pick(sub, idx), ww)
                assert int(o.count.item()) == len(on)
                assert api._secret_residue(p)[0] == 0
        for i in (0, 7, n - 1):
            r = P.decrypt_party_sum(cts, parties[i].secret_key, i, v, plain_modulus=q0, wide=True)
            same(("sum host", vi, i), (r.residues, r.noise, r.status, wide_of(r, W)), pick(ref, i), W)
            col = c2n[:, i].contiguous()
            for resident in (False, True):
                o = Out(1, W)
                torch.cuda.synchronize()
                if resident:
                    with P.DeviceSecretKey(parties[i].secret_key) as key:
                        key.decrypt_sum_device_checked(c1n, col, D, o.out, d_valid=dv, d_noise=o.noise, d_status=o.status, d_count=o.count,
                                                       stream=torch.cuda.current_stream(), plain_modulus=q0, wide=o.wide, wide_words=W)
                        got = o.rows()
                else:
                    sk = dev(sk_all[i])
                    p._call("pvw_decrypt_sum_plain_device", ptr(sk), ptr(c1n), ptr(col), D, ptr(dv), P.REPR_NTT, None, ptr(o.out),
                            ptr(o.noise), ptr(o.status), ptr(o.count), q0, W, ptr(o.wide), cur())
                    got = o.rows()
                same(("sum device", vi, i, resident), got, pick(ref, i), W)
                assert api._secret_residue(p)[0] == 0
        print(f"aggregate mask {vi} ok", flush=True)
    # an all-zero mask on the device forms: nothing is summed, the aggregate is the zero ciphertext, P = 0
    zero = dev(np.zeros(D, np.uint8))
    o = Out(n, W)
    sk = dev(sk_all)
    torch.cuda.synchronize()
    p._call("pvw_decrypt_all_sum_plain_device", 0, n, ptr(sk), ptr(c1n), ptr(c2n), D, ptr(zero), P.REPR_NTT, ptr(o.out), ptr(o.noise),
            ptr(o.status), ptr(o.count), q0, W, ptr(o.wide), cur())
    out, noise, status, wide = o.rows()
    assert not out.any() and not noise.any() and not status.any() and not wide.any() and int(o.count.item()) == 0
    o = Out(1, W)
    sk = dev(sk_all[3])
    col = c2n[:, 3].contiguous()
    torch.cuda.synchronize()
    p._call("pvw_decrypt_sum_plain_device", ptr(sk), ptr(c1n), ptr(col), D, ptr(zero), P.REPR_NTT, None, ptr(o.out), ptr(o.noise),
            ptr(o.status), ptr(o.count), q0, W, ptr(o.wide), cur())
    out, noise, status, wide = o.rows()
    assert not out.any() and not noise.any() and not status.any() and not wide.any() and int(o.count.item()) == 0
    assert api._secret_residue(p)[0] == 0
    print("aggregate ok", flush=True)


def perdealer():
    """pvw_decrypt_batch_plain* and pvw_decrypt_all_plain* on honest single- and multi-dealer ciphertexts, a tampered c2, a wrong
    key; a share encrypted from a negative i64 comes back as its residue with PVW_DEC_NEGATIVE"""
    n, k, l = 24, 32, 8
    moduli = M.bench_moduli(5)
    p, gpk, parties = system(moduli, n, k, l)
    q0 = int(moduli[0])
    W = (p.q_total().bit_length() + 63) // 64
    rng = np.random.default_rng(5)
    for D in (1, n):
        shares, cts = deal(p, gpk, D, n, q0, rng, base=100)
        shares = shares.astype(object)
        shares[0][2] = (1 << 64) - 5                                          # -5 as encode_scalar(i64) reads it
        shares[0][3] = (1 << 64) - 2000
        cts[0] = P.encrypt([int(x) for x in shares[0]], gpk, api._dealer_seed(SEED, 100))
        bad = P.PvwCiphertext(cts[-1].c1.copy(), cts[-1].c2.copy(), p, cts[-1].repr)    # a tampered c2 row
        e = np.zeros((p.L, p.l), dtype=np.uint64)
        e[:, 1] = [(1 << 70) % q for q in p.moduli()]
        qq = np.array(p.moduli(), dtype=object)[:, None]
        bad.c2[4] = ((bad.c2[4].astype(object) + p.ntt_forward(e).astype(object)) % qq).astype(np.uint64)
        cts2 = cts[:-1] + [bad] if D > 1 else cts
        keys = [pt.secret_key for pt in parties]
        keys[5] = parties[6].secret_key                                       # a wrong key for party 5
        nz = np.stack([api._decrypt_batch(p, cts2, keys[i], i, True)[1] for i in range(n)])
        for modulus, ww in ((q0, W), (1000, 0), (0, 1)):
            ref = P.decode_scalar_pvw_plain_host(p, nz.reshape(n * D, p.L, p.l), modulus, ww)
            rv = lambda a: a.reshape(n, D)
            if modulus == q0:
                assert int(rv(ref.residues)[2][0]) == q0 - 5 and int(rv(ref.status)[2][0]) == LOSSY | NEG
                assert int(rv(ref.values)[3][0]) == -2000 and int(rv(ref.residues)[3][0]) == q0 - 2000
                assert (rv(ref.noise)[5] == U64).all()                            # the wrong key
                assert D == 1 or int(rv(ref.noise)[4][D - 1]) == U64              # the tampered row
                for i in range(n):
                    for d in range(D):
                        if i == 5 or (d == 0 and i in (2, 3)) or (D > 1 and (i, d) == (4, D - 1)):
                            continue
                        assert int(rv(ref.residues)[i][d]) == int(shares[d][i]) == int(rv(ref.values)[i][d]), (i, d)
                        assert int(rv(ref.status)[i][d]) == 0 and int(rv(ref.noise)[i][d]) <= p.noise_bound(), (i, d)
            c1n, c2n = dev(np.stack([c.c1 for c in cts2])), dev(np.stack([c.c2 for c in cts2]))
            for lo, cnt in ((1, 6), (0, n)):                                  # both sides of the 22-party dispatch
                idx = (np.arange(lo, lo + cnt)[:, None] * D + np.arange(D)[None, :]).ravel()
                r = P.decrypt_many_checked(cts2, keys[lo:lo + cnt], lo, plain_modulus=modulus or None, wide=bool(ww)) if ww in (0, W) else None
                if r is not None:
                    same(("all host", D, lo, modulus, ww), (r.residues, r.noise, r.status, wide_of(r, ww)), pick(ref, idx), ww)
                o = Out((cnt, D), ww)
                sk = dev(np.stack([kk.secret_coeffs for kk in keys[lo:lo + cnt]]).astype(np.int64))
                torch.cuda.synchronize()
                p._call("pvw_decrypt_all_plain_device", lo, lo + cnt, ptr(sk), ptr(c1n), ptr(c2n), D, P.REPR_NTT, ptr(o.out), ptr(o.noise),
                        ptr(o.status), modulus, ww, ptr(o.wide), cur())
                same(("all device", D, lo, modulus, ww), o.rows(), pick(ref, idx), ww)
                assert api._secret_residue(p)[0] == 0
            for i in (2, 4, 5):
                idx = i * D + np.arange(D)
                if ww in (0, W):
                    r = api._decrypt_batch_checked(p, cts2, keys[i], i, p.noise_bound(), modulus or None, bool(ww))
                    same(("batch host", D, i, modulus, ww), (r.residues, r.noise, r.status, wide_of(r, ww)), pick(ref, idx), ww)
                col = c2n[:, i].contiguous()
                for resident in (False, True):
                    o = Out(D, ww)
                    scratch = torch.zeros((D, p.L, p.l), dtype=torch.int64, device=DEV)
                    torch.cuda.synchronize()
                    if resident:
                        with P.DeviceSecretKey(keys[i]) as key:
                            key.decrypt_device_checked(c1n, col, D, scratch, o.out, o.noise, o.status, torch.cuda.current_stream(),
                                                       plain_modulus=modulus, wide=o.wide if ww else None, wide_words=ww)
                            got = o.rows()
                    else:
                        sk = dev(keys[i].secret_coeffs.astype(np.int64))
                        p._call("pvw_decrypt_batch_plain_device", ptr(sk), ptr(c1n), ptr(col), D, P.REPR_NTT, ptr(scratch), ptr(o.out),
                                ptr(o.noise), ptr(o.status), modulus, ww, ptr(o.wide), cur())
                        got = o.rows()
                    same(("batch device", D, i, resident, modulus, ww), got, pick(ref, idx), ww)
                    assert api._secret_residue(p)[0] == 0
        print(f"perdealer D={D} ok", flush=True)


def capture():
    """after pvw_prepare(PVW_PREPARE_SUM) captured pvw_decrypt_sum_device_sk_plain and pvw_decrypt_all_sum_plain_device replay with
    a changed mask and give the new sums (wide at wide_words = W: the prepared scratch covers it); without pvw_prepare the
    calls are refused and the capture survives"""
    lib = _ffi.lib()
    n, k, l, D = 24, 32, 8, 40
    moduli = M.bench_moduli(5)
    p, gpk, parties = system(moduli, n, k, l)
    q0 = int(moduli[0])
    W = (p.q_total().bit_length() + 63) // 64
    shares, cts = deal(p, gpk, D, n, q0, np.random.default_rng(3))
    i = 3
    c1, c2 = dev(np.stack([c.c1 for c in cts])), dev(np.stack([c.c2 for c in cts]))
    col = c2[:, i].contiguous()
    sk = dev(np.stack([pt.secret_key.secret_coeffs for pt in parties]).astype(np.int64))
    mask = torch.ones(D, dtype=torch.uint8, device=DEV)
    one, every = Out(1, W), Out(n, W)
    with P.DeviceSecretKey(parties[i].secret_key) as key:
        def enqueue(cs):
            rc1 = lib.pvw_decrypt_sum_device_sk_plain(p._h, key._h, ptr(c1), ptr(col), D, ptr(mask), P.REPR_NTT, None, ptr(one.out),
                                                      ptr(one.noise), ptr(one.status), ptr(one.count), q0, W, ptr(one.wide), cs)
            m1 = _ffi.last_error(lib)
            rc2 = lib.pvw_decrypt_all_sum_plain_device(p._h, 0, n, ptr(sk), ptr(c1), ptr(c2), D, ptr(mask), P.REPR_NTT, ptr(every.out),
                                                       ptr(every.noise), ptr(every.status), ptr(every.count), q0, W, ptr(every.wide), cs)
            return rc1, m1, rc2, _ffi.last_error(lib)
        s0 = torch.cuda.Stream(device=DEV)                                    # not prepared: a stream the context has never seen
        torch.cuda.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s0):
            rc1, m1, rc2, m2 = enqueue(cur())
        torch.cuda.synchronize()
        assert rc1 == 1 and "pvw_prepare" in m1 and rc2 == 1 and "pvw_prepare" in m2, (rc1, m1, rc2, m2)
        del g0
        s = torch.cuda.Stream(device=DEV)
        p.prepare(P.PREPARE_SUM, s.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc1, m1, rc2, m2 = enqueue(cur())
        assert rc1 == 0 and rc2 == 0, (m1, m2)
        for rep, v in enumerate((np.ones(D, bool), np.arange(D) % 2 == 0, np.arange(D) == 7)):
            mask.copy_(torch.from_numpy(v.astype(np.uint8)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            ref, _ = refs_of(p, host_sum(p, cts, v), parties, q0, W)
            sums = [sum(int(shares[d][j]) for d in range(D) if v[d]) for j in range(n)]
            assert [int(x) for x in ref.values] == sums
            same(("capture one", rep), one.rows(), pick(ref, i), W)
            same(("capture every", rep), every.rows(), ref, W)
            assert int(one.count.item()) == int(every.count.item()) == int(v.sum())
        del g
    assert api._secret_residue(p)[0] == 0
    print("capture ok", flush=True)


def shard():
    """a sharded context decrypts its parties' aggregate shares to the words of the unsharded one"""
    n, k, l, D = 12, 8, 16, 20
    moduli = M.bench_moduli(5)
    p, gpk, parties = system(moduli, n, k, l)
    part = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).set_shard(4, 9, 2, 6).build()
    q0 = int(moduli[0])
    W = (p.q_total().bit_length() + 63) // 64
    shares, cts = deal(p, gpk, D, n, q0, np.random.default_rng(2))
    valid = np.arange(D) % 4 != 2
    ref, _ = refs_of(p, host_sum(p, cts, valid), parties, q0, W)
    c1s, c2s = np.stack([c.c1 for c in cts]), np.stack([c.c2 for c in cts])
    sk = np.ascontiguousarray(np.stack([pt.secret_key.secret_coeffs for pt in parties[4:9]]).astype(np.int64))
    out, noise, status, wide = np.zeros(5, np.uint64), np.zeros(5, np.uint64), np.zeros(5, np.uint32), np.zeros((5, W), np.uint64)
    v8 = valid.astype(np.uint8)
    part._call("pvw_decrypt_all_sum_plain", 4, 9, api._ptr(sk), api._ptr(c1s), api._ptr(c2s), D, api._ptr(v8), cts[0].repr, api._ptr(out),
               api._ptr(noise), api._ptr(status), None, q0, W, api._ptr(wide))
    same("shard host", (out, noise, status, wide), pick(ref, np.arange(4, 9)), W)
    o = Out(5, W)
    d_sk, d1, d2, dv = dev(sk), dev(c1s), dev(c2s), dev(v8)
    torch.cuda.synchronize()
    part._call("pvw_decrypt_all_sum_plain_device", 4, 9, ptr(d_sk), ptr(d1), ptr(d2), D, ptr(dv), P.REPR_NTT, ptr(o.out), ptr(o.noise),
               ptr(o.status), ptr(o.count), q0, W, ptr(o.wide), cur())
    same("shard device", o.rows(), pick(ref, np.arange(4, 9)), W)
    assert [int(x) for x in out] == [sum(int(shares[d][j]) for d in range(D) if valid[d]) % q0 for j in range(4, 9)]
    assert api._secret_residue(part)[0] == 0
    print("shard ok", flush=True)


CASES = {f.__name__: f for f in (decode, aggregate, perdealer, capture, shard)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]]()
    print("PLAIN_DECODE_OK")

"""Wire format v1 on the device: the codec kernels against the host codec, output into pvw_host_alloc memory, the
rejection count, keys and ciphertexts moved between contexts as bytes.  torch is imported FIRST so both libraries share one
HIP runtime.  Spawned by tests/test_gpu_wire.py; prints WIRE_OK at the end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from pvw_rs_amd import workloads as W  # noqa: E402
from _util import EXAMPLE_MODULI, TEST_MODULI  # noqa: E402
from test_wire_host import _corrupt, chains, params, reduce, words  # noqa: E402

SEED = bytes([0x61]) * 32
VP = C.c_void_p


def dptr(t):
    return VP(t.data_ptr())


def call(p, name, *args):
    rc = getattr(p._lib, name)(p._h, *args)
    assert rc == 0, (name, _ffi.last_error(p._lib))


def device_pack(p, a):
    d = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    out = torch.zeros(len(a) * p.wire_poly_bytes() + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(p, "pvw_wire_pack_device", dptr(d), len(a), dptr(out), None)
    p.synchronize()
    return out[:len(a) * p.wire_poly_bytes()].cpu().numpy().tobytes()


def device_unpack(p, data, count):
    d = torch.from_numpy(np.frombuffer(data + bytes(16), dtype=np.uint8).copy()).cuda()
    out = torch.zeros(count * p.L * p.l + 2, dtype=torch.int64, device="cuda")
    bad = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call(p, "pvw_wire_unpack_device", dptr(d), count, dptr(out), dptr(bad), None)
    p.synchronize()
    return out[:count * p.L * p.l].cpu().numpy().view(np.uint64).reshape(count, p.L, p.l), int(bad[0])


def check_codec():
    rng = np.random.default_rng(5)
    n = 0
    for l in (8, 16, 32, 64):
        for name, moduli in chains(l).items():
            p = params(moduli, l)
            for count in (1, 15, 16, 17, 300):
                a = words(rng, count, moduli, l)
                host = api.wire_pack_host(p, a)
                assert device_pack(p, a) == host == api.wire_pack(p, a), (name, l, count)
                back, bad = device_unpack(p, host, count)
                assert bad == 0 and np.array_equal(back, a), (name, l, count)
                assert np.array_equal(api.wire_unpack(p, host, count), a)
                u = words(rng, count, moduli, l, unreduced=True)
                assert device_pack(p, u) == api.wire_pack_host(p, reduce(u, moduli)), (name, l, count, "unreduced")
                n += 1
    print(f"codec: {n} (chain, l, count) cases bit-identical to the host codec")


def check_large():
    # >= 256 MB of words, unreduced: a seeded sample of polynomials plus the first and the last against the host codec
    p = params(W.bench_moduli(17), 8)
    P_ = p.L * p.l
    count = (272 << 20) // (P_ * 8)
    pb = p.wire_poly_bytes()
    g = torch.Generator(device="cuda").manual_seed(11)
    d = torch.randint(0, (1 << 63) - 1, (count * P_,), dtype=torch.int64, device="cuda", generator=g)
    out = torch.zeros(count * pb + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(p, "pvw_wire_pack_device", dptr(d), count, dptr(out), None)
    p.synchronize()
    idx = sorted(set(np.random.default_rng(3).choice(count, 300, replace=False).tolist()) | {0, count - 1})
    sel = torch.tensor(idx, device="cuda")
    w = d.view(count, P_)[sel].cpu().numpy().view(np.uint64).reshape(len(idx), p.L, p.l)
    ob = out[:count * pb].view(count, pb)[sel].cpu().numpy()
    for i, x in enumerate(idx):
        assert ob[i].tobytes() == api.wire_pack_host(p, w[i:i + 1]), x
    back = torch.zeros(count * P_ + 2, dtype=torch.int64, device="cuda")
    bad = torch.zeros(2, dtype=torch.int64, device="cuda")
    call(p, "pvw_wire_unpack_device", dptr(out), count, dptr(back), dptr(bad), None)
    p.synchronize()
    assert int(bad[0]) == 0
    r = back[:count * P_].view(count, P_)[sel].cpu().numpy().view(np.uint64).reshape(len(idx), p.L, p.l)
    assert np.array_equal(r, reduce(w, p.moduli()))
    # into pvw_host_alloc memory: the same bytes
    m = 20000
    host = VP()
    assert p._lib.pvw_host_alloc(m * pb, C.byref(host)) == 0
    try:
        call(p, "pvw_wire_pack_device", dptr(d), m, host, None)
        p.synchronize()
        assert C.string_at(host, m * pb) == out[:m * pb].cpu().numpy().tobytes()
        # pvw_wire_pack with a pvw_host_alloc destination (the kernel writes it directly)
        src = d[:m * P_].cpu().numpy().view(np.uint64)
        call(p, "pvw_wire_pack", src.ctypes.data_as(VP), m, host)
        assert C.string_at(host, m * pb) == out[:m * pb].cpu().numpy().tobytes()
    finally:
        p._lib.pvw_host_free(host)
    del d, out, back
    torch.cuda.empty_cache()
    print(f"large: {count} polynomials ({count * P_ * 8 >> 20} MiB of words), {len(idx)} sampled, host-memory output identical")


def check_rejection_count():
    rng = np.random.default_rng(9)
    for l, moduli in ((8, TEST_MODULI), (16, EXAMPLE_MODULI), (64, chains(64)["mixed"])):
        p = params(moduli, l)
        a = words(rng, 40, moduli, l)
        data = api.wire_pack_host(p, a)
        planted = set()
        while len(planted) < 37:
            planted.add((int(rng.integers(40)), int(rng.integers(len(moduli))), int(rng.integers(l))))
        for (pp, i, j) in planted:
            q = moduli[i]
            data = _corrupt(data, moduli, l, pp, i, j, q if (pp + j) % 2 else (1 << q.bit_length()) - 1)
        back, bad = device_unpack(p, data, 40)
        assert bad == 37, bad
        for (pp, i, j) in planted:
            assert int(back[pp, i, j]) >= moduli[i]
        try:
            api.wire_unpack(p, data, 40)
            raise AssertionError("accepted")
        except P.PvwError as e:
            assert e.variant == "DeserializationError"
            first = min(planted)
            assert f"polynomial {first[0]}, limb {first[1]}, slot {first[2]}" in str(e), (str(e), first)
    print("rejection: 37 planted residues counted on the device, the first one named")


def system(n, k, l, moduli, shard=None, keygen=True):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if shard:
        b = b.set_shard(*shard)
    p = b.build()
    crs = P.PvwCrs.new_deterministic(p, SEED)
    gpk = P.GlobalPublicKey.new(crs)
    parties = []
    if keygen:
        parties = [P.Party.new(i, p, SEED) for i in range(n)]
        gpk.generate_all_party_keys(parties, SEED)
    return p, crs, gpk, parties


def check_keys():
    n, k, l = 32, 64, 8
    pa, crs_a, gpk_a, _ = system(n, k, l, EXAMPLE_MODULI)
    for repr in (P.REPR_POWER, P.REPR_NTT):
        # get vs load: the packed rows equal host packing of pvw_get_pk / pvw_get_crs
        blob = gpk_a.to_bytes(repr=repr)
        _, rg, hl, _ = api._wire_check(pa, blob, _ffi.WIRE_PK)
        assert rg[:2] == (0, n) and blob[hl:] == api.wire_pack_host(pa, gpk_a.matrix(repr=repr).reshape(-1, pa.L, l))
        sub = gpk_a.to_bytes(5, 9, repr=repr)
        assert sub[api._wire_check(pa, sub, _ffi.WIRE_PK)[2]:] == api.wire_pack_host(pa, gpk_a.matrix(5, 9, repr).reshape(-1, pa.L, l))
        cb = crs_a.to_bytes(repr)
        assert cb[api._wire_check(pa, cb, _ffi.WIRE_CRS)[2]:] == api.wire_pack_host(pa, crs_a.matrix(repr).reshape(-1, pa.L, l))
        # load from bytes vs pvw_load_pk of the same key: identical encrypts on the packed-stream and the matrix-core paths
        pb_, crs_b, gpk_b, _ = system(n, k, l, EXAMPLE_MODULI, keygen=False)
        gpk_b.load_bytes(blob)
        pc, crs_c, gpk_c, _ = system(n, k, l, EXAMPLE_MODULI, keygen=False)
        gpk_c.load_rows(0, gpk_a.matrix(repr=repr), repr)
        pd, _, _, _ = system(n, k, l, EXAMPLE_MODULI, keygen=False)
        P.PvwCrs.from_bytes(pd, cb)
        assert np.array_equal(P.PvwCrs(pd).matrix(P.REPR_NTT), crs_a.matrix(P.REPR_NTT))
        assert gpk_b.num_public_keys() == n
        outs = []
        for p, g in ((pb_, gpk_b), (pc, gpk_c)):
            p.prepare()
            assert p.packed_active() > 0
            sc = [(7 * i + 3) % (1 << 32) for i in range(n)]
            ct = P.encrypt(sc, g, SEED)
            cts = P.encrypt_all_party_shares([[d * n + j for j in range(n)] for d in range(n)], g, SEED)
            outs.append((ct, cts))
        (c0, m0), (c1, m1) = outs
        assert np.array_equal(c0.c1, c1.c1) and np.array_equal(c0.c2, c1.c2)
        assert all(np.array_equal(x.c2, y.c2) and np.array_equal(x.c1, y.c1) for x, y in zip(m0, m1))
        # atomic rejection: nothing changes, the next encrypt is bit-identical
        bad = bytearray(blob)
        bad[-3:] = b"\xff\xff\xff"
        before = P.encrypt([1] * n, gpk_b, SEED)
        try:
            gpk_b.load_bytes(bytes(bad))
            raise AssertionError("corrupted key accepted")
        except P.PvwError as e:
            assert e.variant == "DeserializationError", e
        after = P.encrypt([1] * n, gpk_b, SEED)
        assert np.array_equal(before.c2, after.c2) and np.array_equal(before.c1, after.c1)
        assert pb_.packed_active() > 0                                  # the derived copies were not invalidated
        # ... and num_public_keys stays where it was
        pe, _, gpk_e, _ = system(n, k, l, EXAMPLE_MODULI, keygen=False)
        gpk_e.load_bytes(gpk_a.to_bytes(0, 16, repr))
        assert gpk_e.num_public_keys() == 16
        try:
            gpk_e.load_bytes(bytes(bad))
            raise AssertionError("corrupted key accepted")
        except P.PvwError:
            pass
        assert gpk_e.num_public_keys() == 16
    print("keys: get == host pack, load_bytes == load_pk on both encrypt paths, rejected loads change nothing")


def check_end_to_end():
    n, k, l = 16, 4, 16
    bounds = P.PvwParameters.suggest_error_bounds(n, k, l, TEST_MODULI, 0.5)

    def ctx():
        return (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(TEST_MODULI)
                .set_error_bounds(*bounds).build())
    pa, pb_ = ctx(), ctx()
    crs_a = P.PvwCrs.new_deterministic(pa, SEED)
    gpk_a = P.GlobalPublicKey.new(crs_a)
    parties = [P.Party.new(i, pa, SEED) for i in range(n)]
    gpk_a.generate_all_party_keys(parties, SEED)
    shares = [[(d * 1000 + j + 1) for j in range(n)] for d in range(n)]
    cts = P.encrypt_all_party_shares(shares, gpk_a, SEED)
    # second context: parameters, CRS and public key all arrive as bytes
    pb_ = P.PvwParameters.from_bytes(pa.to_bytes())
    crs_b = P.PvwCrs.from_bytes(pb_, crs_a.to_bytes())
    gpk_b = P.GlobalPublicKey.from_bytes(crs_b, gpk_a.to_bytes())
    back = [P.PvwCiphertext.from_bytes(pb_, ct.to_bytes()) for ct in cts]
    assert all(np.array_equal(x.c1, y.c1) and np.array_equal(x.c2, y.c2) and x.repr == y.repr for x, y in zip(back, cts))
    keys = [P.Party(pt.index, P.SecretKey.from_bytes(pb_, pt.secret_key.to_bytes())) for pt in parties]
    res = P.decrypt_all_party_shares(back, keys)
    assert [[int(res[i][d]) for d in range(n)] for i in range(n)] == [[shares[d][i] for d in range(n)] for i in range(n)]
    chk = P.decrypt_all_party_shares_checked(back, keys)
    assert bool(np.all(chk.valid)), chk
    # the moved key encrypts what the original does
    again = P.encrypt_all_party_shares(shares, gpk_b, SEED)
    assert all(np.array_equal(x.c2, y.c2) for x, y in zip(again, cts))
    print("end to end: ciphertexts and key moved as bytes decrypt to the dealt values, every share valid")


def check_shard():
    n, k, l = 24, 8, 8
    pf, crs_f, gpk_f, _ = system(n, k, l, TEST_MODULI)
    pf2 = P.PvwParameters.from_bytes(pf.to_bytes())
    ps = (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(TEST_MODULI)
          .set_shard(8, 16, 0, k).build())
    crs_s = P.PvwCrs.new_deterministic(ps, SEED)
    gpk_s = P.GlobalPublicKey.new(crs_s)
    gpk_s.load_bytes(gpk_f.to_bytes())                     # rows outside the shard are not read
    blob_s = gpk_s.to_bytes()
    assert api._wire_check(ps, blob_s, _ffi.WIRE_PK)[1][:2] == (8, 16)
    assert blob_s == gpk_f.to_bytes(8, 16)
    sc = [3 * i + 1 for i in range(n)]
    ct_f, ct_s = P.encrypt(sc, gpk_f, SEED), P.encrypt(sc, gpk_s, SEED)
    bs = ct_s.to_bytes()
    assert api._wire_check(ps, bs, _ffi.WIRE_CT)[1] == (0, k, 8, 16)
    assert bs == ct_f.to_bytes(8, 16)
    back = P.PvwCiphertext.from_bytes(pf2, bs)
    assert np.array_equal(back.c2[8:16], ct_f.c2[8:16]) and not back.c2[:8].any() and np.array_equal(back.c1, ct_f.c1)
    print("shard: key and ciphertext blobs of the shard's party range equal the full context's")


def check_cpp():
    exe = os.path.join(ROOT, "build", "wire_roundtrip")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "pvw_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "wire_roundtrip.cpp"), "-o", exe,
                           "-L" + lib, "-lpvw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "WIRE_CPP_OK" in out.stdout, out.stdout + out.stderr
    print("c++ mirror: " + out.stdout.strip())


if __name__ == "__main__":
    assert P.device_available()
    for step in (check_codec, check_rejection_count, check_large, check_keys, check_end_to_end, check_shard, check_cpp):
        step()
        sys.stdout.flush()
    print("WIRE_OK")

"""Key generation from a seed on the device: pvw_keygen_seeded -- the drawn shat_mftile_kernel on the swapped
matrix-core path, the sampled `js` prologue family at l = 64 and on the transposed / VALU paths --, pvw_sample_secret_keys_device
and pvw_sk_load_seeded, bit for bit against the C oracle on the oracle's own draw of the keys and against the two-step device
path (pvw_sample_secret_keys + pvw_keygen).  torch is imported FIRST so both libraries share one HIP runtime.  Spawned case by
case by tests/test_gpu_keygen_seeded.py; prints KEYGEN_SEEDED_OK."""
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
import pvw_oracle as O  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import primes_1mod  # noqa: E402

SK_SEED, SEED, FILL = bytes([0x3D]) * 32, bytes([0x5A]) * 32, bytes([0x77]) * 32
# (n, k, l, L): one shape per branch of pvw_keygen_seeded
SHAPES = {
    "valu": (5, 12, 8, 2),              # below 8 parties: four per pass on the VALU, the sampled js family into w->rhat
    "k1": (5, 1, 8, 2),                 # k = 1
    "transposed": (40, 24, 8, 2),       # 8..63 parties: transposed GEMM, the sampled js family into the vector layout
    "swapped": (70, 9, 8, 3),           # from 64 parties: the drawn shat_mftile, ragged rows (70 of 96) and ragged k (9 of 16)
    "l32": (70, 12, 32, 2),             # l = 32: the widest drawn instantiation
    "l64": (70, 8, 64, 2),              # l = 64 at >= 64 parties: the prologue branch of the swapped path
    "chunks": (1100, 32, 16, 2),        # two chunks of parties, the second ragged (76): party0 of the second draw
}


def moduli_for(l, L):
    return primes_1mod(128, L) if l == 64 else M.bench_moduli(L)


def params(n, k, l, moduli, variance=0.5, bounds=(100, 200), shard=None):
    b = (P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
         .set_secret_variance(variance).set_error_bounds(*bounds))
    if shard:
        b.set_shard(*shard)
    return b.build()


def oracle_rows(crs, moduli, n, k, l, sk_seed, seed, variance=0.5, b1=100, lo=0, hi=None):
    """the C oracle's B-hat rows [lo, hi) from ITS OWN draw of the keys: global stream indices p * k + j"""
    hi = n if hi is None else hi
    sk = O.sample_cbd(sk_seed, M.DOM_SK, lo * k, (hi - lo) * k, l, variance).reshape(hi - lo, k, l)
    ek = O.sample_uniform(seed, M.DOM_EKEY, lo * k, (hi - lo) * k, l, b1).reshape(hi - lo, k, l)
    return O.Oracle(moduli, l).keygen(crs.matrix(P.REPR_NTT), sk, ek)


def two_step(p, crs, lo, hi, sk_seed, seed):
    """pvw_sample_secret_keys + pvw_keygen(ek = NULL) on a key of its own: rows [lo, hi)"""
    gpk = P.GlobalPublicKey.new(crs)
    sk = np.zeros((hi - lo, p.k, p.l), dtype=np.int64)
    p._call("pvw_sample_secret_keys", api._ptr(api._seed(sk_seed)), lo, hi - lo, api._ptr(sk))
    gpk._keygen(lo, hi, sk, None, seed)
    return gpk.matrix(lo, hi, P.REPR_NTT)


def residue_clean(p):
    nz, scanned = api._secret_residue(p)
    assert nz == 0 and scanned > 0, (nz, scanned)


def path_case(n, k, l, L, variance=0.5, bounds=(100, 200)):
    moduli = moduli_for(l, L)
    for sk_seed in (SK_SEED, SEED):                                   # distinct seeds, then one seed for both domains
        p = params(n, k, l, moduli, variance, bounds)
        crs = P.PvwCrs.new_deterministic(p, SEED)
        gpk = P.GlobalPublicKey.new(crs)
        gpk.generate_seeded(0, n, sk_seed, SEED)
        got = gpk.matrix(repr=P.REPR_NTT)
        residue_clean(p)
        assert gpk.num_public_keys() == n and gpk.is_full()
        want = oracle_rows(crs, moduli, n, k, l, sk_seed, SEED, variance, bounds[0])
        assert np.array_equal(got, want), f"({n}, {k}, {l}, {L}) variance {variance}: B-hat differs from the oracle"
        # two_step rewrites the same resident matrix: read after `got` was taken
        assert np.array_equal(two_step(p, crs, 0, n, sk_seed, SEED), want), "the two-step path differs from the oracle"


def case_range():
    n, k, l, L = 70, 9, 8, 3
    moduli = moduli_for(l, L)
    p, twin = params(n, k, l, moduli), params(n, k, l, moduli)
    crs, crs_t = P.PvwCrs.new_deterministic(p, SEED), P.PvwCrs.new_deterministic(twin, SEED)
    gpk, gpk_t = P.GlobalPublicKey.new(crs), P.GlobalPublicKey.new(crs_t)
    gpk.fill_uniform(FILL)
    gpk_t.fill_uniform(FILL)
    before = gpk.matrix(repr=P.REPR_NTT)
    for lo, hi in ((37, 70), (3, 8)):                                 # swapped (33 rows, party0 = 37) and VALU (5 rows)
        gpk.generate_seeded(lo, hi, SK_SEED, SEED)
        got = gpk.matrix(repr=P.REPR_NTT)
        before[lo:hi] = oracle_rows(crs, moduli, n, k, l, SK_SEED, SEED, lo=lo, hi=hi)
        assert np.array_equal(got, before), f"rows [{lo}, {hi}) or their neighbours"
        residue_clean(p)
        # the bookkeeping is pvw_keygen's
        sk = np.zeros((hi - lo, k, l), dtype=np.int64)
        twin._call("pvw_sample_secret_keys", api._ptr(api._seed(SK_SEED)), lo, hi - lo, api._ptr(sk))
        gpk_t._keygen(lo, hi, sk, None, SEED)
        assert gpk.num_public_keys() == gpk_t.num_public_keys() == n
    assert np.array_equal(gpk_t.matrix(repr=P.REPR_NTT), before)
    # on a key nothing was loaded into: the count is the range's end
    fresh = params(n, k, l, moduli)
    g = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(fresh, SEED))
    g.generate_seeded(3, 8, SK_SEED, SEED)
    assert g.num_public_keys() == 8 and not g.is_full()
    assert np.array_equal(g.matrix(3, 8, P.REPR_NTT), before[3:8])
    g.generate_seeded(5, 5, SK_SEED, SEED)                            # an empty range changes nothing
    assert g.num_public_keys() == 8 and np.array_equal(g.matrix(3, 8, P.REPR_NTT), before[3:8])


def case_variance():
    for variance, bounds in ((1.0, (100, 200)), (3.0, (100, 200)), (10.0, (1, 1172385))):
        path_case(70, 9, 8, 3, variance, bounds)
        path_case(70, 12, 16, 2, variance, bounds)
    path_case(40, 24, 8, 2, 3.0)                                      # ... and through the sampled prologue family
    path_case(70, 8, 64, 2, 3.0)


def case_sharded():
    n, k, l, L = 70, 9, 8, 3
    moduli = moduli_for(l, L)
    full = params(n, k, l, moduli)
    g = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(full, SEED))
    g.generate_seeded(0, n, SK_SEED, SEED)
    want = g.matrix(repr=P.REPR_NTT)
    for lo, hi in ((2, 69), (20, 60), (61, 66)):                      # swapped from party 2, transposed, VALU
        ps = params(n, k, l, moduli, shard=(lo, hi, 0, k))            # key generation needs the full CRS
        gs = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(ps, SEED))
        gs.generate_seeded(0, n, SK_SEED, SEED)
        got = gs.matrix(repr=P.REPR_NTT)
        assert np.array_equal(got[lo:hi], want[lo:hi]), f"held rows [{lo}, {hi})"
        assert not got[:lo].any() and not got[hi:].any()
        assert gs.num_public_keys() == n
        residue_clean(ps)


def case_tuning():
    prev = _ffi.select("tuning")
    try:
        for env in ({"PVW_KEYGEN_SWAP": "0"}, {"PVW_GEMM_MIN_DEALERS": "0"}):
            os.environ.update(env)
            try:
                assert params(3, 4, 8, moduli_for(8, 2))._lib.pvw_build_is_tuning() == 1
                path_case(150, 256, 8, 2)
                path_case(70, 9, 8, 3)
            finally:
                for name in env:
                    del os.environ[name]
    finally:
        _ffi.select(prev)


def _dealt(n, k, l, L):
    """a seeded key, n dealers' ciphertexts under it and the shares dealt: (p, c1s [n][k][L][l], c2s [n][n][L][l], rows)"""
    moduli = moduli_for(l, L)
    b1, b2 = P.PvwParameters.suggest_error_bounds(n, k, l, moduli, 0.5)
    p = params(n, k, l, moduli, 0.5, (b1, b2))
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.generate_seeded(0, n, SK_SEED, SEED)
    rows = [[d * 100 + j for j in range(1, n + 1)] for d in range(n)]
    cts = P.encrypt_all_party_shares(rows, gpk, SEED)
    return p, np.stack([ct.c1 for ct in cts]), np.stack([ct.c2 for ct in cts]), np.array(rows, dtype=np.uint64)


def case_sk_device():
    n, k, l, L, D = 24, 16, 8, 5, 3
    p, c1s, c2s, rows = _dealt(n, k, l, L)
    dev = torch.device("cuda", 0)
    c1s, c2s = np.ascontiguousarray(c1s[:D]), np.ascontiguousarray(c2s[:D])
    d_c1, d_c2 = torch.from_numpy(c1s.view(np.int64)).to(dev), torch.from_numpy(c2s.view(np.int64)).to(dev)
    seed_np = api._seed(SK_SEED)
    for lo, hi in ((0, 24), (3, 8)):                                  # 24 parties x 3 dealers on the matrix cores, 5 parties below them
        cnt = hi - lo
        sk = np.full((cnt, k, l), 99, dtype=np.int64)
        p._call("pvw_sample_secret_keys", api._ptr(seed_np), lo, cnt, api._ptr(sk))
        assert np.array_equal(sk, O.sample_cbd(SK_SEED, M.DOM_SK, lo * k, cnt * k, l, 0.5).reshape(cnt, k, l))
        d_sk = P.sample_secret_keys_device(p, SK_SEED, lo, cnt)
        torch.cuda.synchronize()
        assert d_sk.shape == (cnt, k, l) and np.array_equal(d_sk.cpu().numpy(), sk), f"keys of parties [{lo}, {hi})"
        # into a caller's tensor on a caller's stream, beside words that stay
        s = torch.cuda.Stream(device=dev)
        buf = torch.full((cnt + 1, k, l), 7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert P.sample_secret_keys_device(p, SK_SEED, lo, cnt, out=buf[:cnt], stream=s) is not None
        s.synchronize()
        assert np.array_equal(buf[:cnt].cpu().numpy(), sk) and bool((buf[cnt] == 7).all())
        want = np.zeros((cnt, D), dtype=np.uint64)
        p._call("pvw_decrypt_all", lo, hi, api._ptr(sk), api._ptr(c1s), api._ptr(c2s), D, P.REPR_NTT, api._ptr(want))
        d_out = torch.zeros((cnt, D), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        p._call("pvw_decrypt_all_device", lo, hi, api._dptr(d_sk), api._dptr(d_c1), api._dptr(d_c2), D, P.REPR_NTT, api._dptr(d_out), None)
        p.synchronize()
        got = d_out.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), f"pvw_decrypt_all_device fed with drawn keys, parties [{lo}, {hi})"
        assert (got == rows[:D, lo:hi].T).mean() >= 0.95
        d_sk.zero_()
        buf.zero_()
    torch.cuda.synchronize()
    with np.testing.assert_raises(P.PvwError):
        P.sample_secret_keys_device(p, SK_SEED, 0, 2, out=torch.zeros(5, dtype=torch.int64, device=dev))


def case_resident():
    n, k, l, L = 12, 6, 8, 3
    p, c1s, c2s, rows = _dealt(n, k, l, L)
    dev = torch.device("cuda", 0)
    lib = p._lib
    d_c1 = torch.from_numpy(c1s.view(np.int64)).to(dev)
    for i in (0, 7, n - 1):
        d_c2col = torch.from_numpy(np.ascontiguousarray(c2s[:, i]).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        outs = []
        host_key = P.SecretKey.random(p, SK_SEED, i)
        for key in (host_key.load_device(), P.DeviceSecretKey.from_seed(p, SK_SEED, i)):
            noisy = torch.zeros((n, L, l), dtype=torch.int64, device=dev)
            vals = torch.zeros(n, dtype=torch.int64, device=dev)
            for _ in range(2):                                        # a resident key serves call after call
                api._check(lib.pvw_decrypt_batch_device_sk(p._h, key._h, api._dptr(d_c1), api._dptr(d_c2col), n, P.REPR_NTT,
                                                           api._dptr(noisy), api._dptr(vals), None), lib)
                p.synchronize()
            outs.append((noisy.cpu().numpy(), vals.cpu().numpy().view(np.uint64)))
            key.free()
            assert not key._h
            key.free()                                                # freeing twice is harmless
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), f"party {i}"
        assert (outs[1][1] == rows[:, i]).mean() >= 0.9
    with P.DeviceSecretKey.from_seed(p, SK_SEED, 3) as key:
        assert key._h
    assert not key._h
    residue_clean(p)


def case_hygiene():
    dev = torch.device("cuda", 0)
    for name in ("swapped", "l64", "transposed", "valu", "chunks"):
        n, k, l, L = SHAPES[name]
        p = params(n, k, l, moduli_for(l, L))
        gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
        gpk.generate_seeded(0, n, SK_SEED, SEED)
        residue_clean(p)
        d_sk = P.sample_secret_keys_device(p, SK_SEED, 0, min(n, 9))
        torch.cuda.synchronize()
        residue_clean(p)
        d_sk.zero_()
        key = P.DeviceSecretKey.from_seed(p, SK_SEED, n - 1)
        residue_clean(p)
        key.free()
        residue_clean(p)
        gpk.generate_seeded(n // 2, n, SK_SEED, SEED)                 # again on the workspace the first call left
        residue_clean(p)
    del dev


def case_loop():
    n, k, l, L = 48, 32, 8, 5
    moduli = M.bench_moduli(L)
    p = params(n, k, l, moduli)
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    gpk.generate_seeded(0, n, SK_SEED, SEED)
    assert gpk.is_full()
    scalars = [(i * 1000 + 1) % (1 << 32) for i in range(n)]
    ct = P.encrypt(scalars, gpk, SEED)
    got = [P.decrypt_party_value(ct, P.SecretKey.random(p, SK_SEED, i), i) for i in range(n)]
    assert sum(a == b for a, b in zip(got, scalars)) >= 0.95 * n, got[:6]
    # a key drawn from another seed does not open it
    other = [P.decrypt_party_value(ct, P.SecretKey.random(p, SEED, i), i) for i in range(4)]
    assert other != scalars[:4]


def main():
    case = sys.argv[1]
    assert torch.cuda.is_available() and P.device_available()
    if case.startswith("paths-"):
        path_case(*SHAPES[case[len("paths-"):]])
    else:
        globals()["case_" + case]()
    print("KEYGEN_SEEDED_OK")


if __name__ == "__main__":
    main()

"""Checked decryption on the device against the host implementation that computes each residual by its
definition (pvw_decode_checked_host).  torch is imported FIRST so both libraries share one HIP runtime.  Spawned by
tests/test_gpu_checked_decrypt.py; prints CHECKED_DECRYPT_OK at the end."""
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
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import EXAMPLE_MODULI, TEST_MODULI  # noqa: E402
from test_checked_decode_host import SETS, checked_cases, _rns  # noqa: E402

U64 = (1 << 64) - 1
SEED = bytes([0x2A]) * 32
BIG = (1 << 63) + 5                                      # encoded as a negative i64 by the reference: decodes lossy


def same(a, b, what):
    assert np.array_equal(np.asarray(a.values), np.asarray(b.values)), what + ": values"
    bad = np.nonzero(np.asarray(a.noise) != np.asarray(b.noise))[0]
    assert len(bad) == 0, (what + ": noise", [(int(i), int(a.noise.flat[i]), int(b.noise.flat[i])) for i in bad[:4]])
    assert np.array_equal(np.asarray(a.status), np.asarray(b.status)), what + ": status"


def system(moduli, l, n, k, bounds=None):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    if bounds:
        b = b.set_error_bounds(*bounds)
    p = b.build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(p, SEED))
    parties = [P.Party.new(i, p, SEED) for i in range(n)]
    gpk.generate_all_party_keys(parties, SEED)
    return p, gpk, parties


def check_party(p, cts, key, i, what):
    """the checked call against the unchecked one (values) and against the host definition on the same noisy polynomials"""
    vals, noisy = P.decrypt_party_shares(cts, key, i, return_noisy=True)
    r = P.decrypt_party_shares_checked(cts, key, i)
    assert [int(v) for v in r.values] == vals, what
    same(r, P.decode_scalar_pvw_checked_host(p, noisy), what)
    return r


def honest(name, moduli, l, n, k, bounds=None):
    p, gpk, parties = system(moduli, l, n, k, bounds)
    scal = [[(d * 1009 + i * 31 + 7) % (1 << 32) for i in range(n)] for d in range(n)]
    scal[0][1] = BIG
    single = [P.encrypt(scal[d], gpk, api._dealer_seed(SEED, d)) for d in range(n)]          # one dealer per call
    multi = P.encrypt_many(scal, gpk, [api._dealer_seed(SEED, 100 + d) for d in range(n)])   # multi-dealer (GEMM when wide)
    bound = p.noise_bound()
    for cts, tag in ((single, "encrypt"), (multi, "encrypt_multi")):
        for i in (0, 1, n - 1):
            r = check_party(p, cts, parties[i].secret_key, i, f"{name} {tag} party {i}")
            want = [scal[d][i] for d in range(n)]
            lossy_want = [want[d] == BIG for d in range(n)]
            assert list(r.lossy) == lossy_want, (name, tag, i)
            assert all(int(v) == w for v, w, lo in zip(r.values, want, lossy_want) if not lo), (name, tag, i)
            assert all(int(v) == 0 for v, lo in zip(r.values, lossy_want) if lo), (name, tag, i)    # Q > 2^65
            assert list(r.valid) == [not lo and int(v) <= bound for lo, v in zip(lossy_want, r.noise)]
        print(f"{name} {tag}: honest noise max {int(r.noise.max())} (bound {bound})", flush=True)
    return p, gpk, parties, single, scal


def tampered(p, parties, cts, name):
    n, L, l = p.n, p.L, p.l
    i = 2
    for delta, j in ((1, 0), (-5, 3), (1 << 20, l - 1), (1 << 70, 1), ((1 << 64) + 9, l // 2)):
        bad = [P.PvwCiphertext(ct.c1.copy(), ct.c2.copy(), p, ct.repr) for ct in cts]
        e = np.zeros((L, l), dtype=np.uint64)
        e[:, j] = [delta % q for q in p.moduli()]
        for d in (0, 3):
            add = p.ntt_forward(e) if bad[d].repr == P.REPR_NTT else e
            bad[d].c2[i] = (bad[d].c2[i].astype(object) + add.astype(object)) % np.array(p.moduli(), dtype=object)[:, None]
            bad[d].c2[i] = bad[d].c2[i].astype(np.uint64)
        r = check_party(p, bad, parties[i].secret_key, i, f"{name} tampered {delta} X^{j}")
        if abs(delta) >= 1 << 64:
            assert int(r.noise[0]) == U64 and not r.valid[0], (name, delta)
    r = check_party(p, cts, parties[3].secret_key, 2, f"{name} wrong key")                    # party 3's key at index 2
    assert not r.valid.any(), name
    r = check_party(p, cts, parties[2].secret_key, 4, f"{name} wrong party index")
    assert not r.valid.any(), name
    # nothing of the keys left behind by the checked calls (before a decode reuses the workspace's staging for its input)
    nz, _ = api._secret_residue(p)
    assert nz == 0, (name, nz)
    rng = np.random.default_rng(5)
    uni = np.stack([rng.integers(0, q, size=(64, l), dtype=np.uint64) for q in p.moduli()], axis=1)
    same(P.decode_scalar_pvw_checked(p, uni), P.decode_scalar_pvw_checked_host(p, uni), f"{name} uniform residues")


def many(p, parties, cts, name):
    for lo, cnt in ((1, 5), (0, 24)):                     # both sides of the 22-party dispatch
        keys = [pt.secret_key for pt in parties[lo:lo + cnt]]
        r = P.decrypt_many_checked(cts, keys, lo)
        plain = P.decrypt_many(cts, keys, lo)
        assert np.array_equal(r.values, plain), (name, cnt)
        for row, i in enumerate(range(lo, lo + cnt)):
            ri = P.decrypt_party_shares_checked(cts, parties[i].secret_key, i)
            same(CheckedRow(r, row), ri, f"{name} decrypt_many_checked {cnt} row {row}")
        # device variant on torch buffers
        dev = torch.device("cuda", 0)
        c1 = torch.from_numpy(np.stack([ct.c1 for ct in cts]).view(np.int64)).to(dev)
        c2 = torch.from_numpy(np.stack([ct.c2 for ct in cts]).view(np.int64)).to(dev)
        sk = torch.from_numpy(np.stack([k.secret_coeffs for k in keys]).astype(np.int64)).to(dev)
        out = torch.zeros((cnt, len(cts)), dtype=torch.int64, device=dev)
        nz = torch.zeros_like(out)
        st = torch.zeros((cnt, len(cts)), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p._call("pvw_decrypt_all_checked_device", lo, lo + cnt, C.c_void_p(sk.data_ptr()), C.c_void_p(c1.data_ptr()),
                C.c_void_p(c2.data_ptr()), len(cts), cts[0].repr, C.c_void_p(out.data_ptr()), C.c_void_p(nz.data_ptr()),
                C.c_void_p(st.data_ptr()), stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), r.values), (name, cnt)
        assert np.array_equal(nz.cpu().numpy().view(np.uint64), r.noise), (name, cnt)
        assert np.array_equal(st.cpu().numpy().view(np.uint32), r.status), (name, cnt)
    print(f"{name}: decrypt_many_checked ok", flush=True)


class CheckedRow:
    def __init__(self, r, row):
        self.values, self.noise, self.status = r.values[row], r.noise[row], r.status[row]


def resident_key(p, parties, cts, name):
    dev = torch.device("cuda", 0)
    i = 1
    c1 = torch.from_numpy(np.stack([ct.c1 for ct in cts]).view(np.int64)).to(dev)
    c2 = torch.from_numpy(np.stack([ct.c2[i] for ct in cts]).view(np.int64)).to(dev)
    D = len(cts)
    noisy = torch.zeros((D, p.L, p.l), dtype=torch.int64, device=dev)
    out = torch.zeros(D, dtype=torch.int64, device=dev)
    nz = torch.zeros(D, dtype=torch.int64, device=dev)
    st = torch.zeros(D, dtype=torch.int32, device=dev)
    with P.DeviceSecretKey(parties[i].secret_key) as key:
        key.decrypt_device_checked(c1, c2, D, noisy, out, nz, st, torch.cuda.current_stream())
        torch.cuda.synchronize()
    want = P.decrypt_party_shares_checked(cts, parties[i].secret_key, i)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want.values), name
    assert np.array_equal(nz.cpu().numpy().view(np.uint64), want.noise), name
    assert np.array_equal(st.cpu().numpy().view(np.uint32), want.status), name
    # the key-upload device variant
    sk = torch.from_numpy(np.asarray(parties[i].secret_key.secret_coeffs, dtype=np.int64)).to(dev)
    out2, nz2, st2 = torch.zeros_like(out), torch.zeros_like(nz), torch.zeros_like(st)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p._call("pvw_decrypt_batch_checked_device", C.c_void_p(sk.data_ptr()), C.c_void_p(c1.data_ptr()), C.c_void_p(c2.data_ptr()), D,
            cts[0].repr, C.c_void_p(noisy.data_ptr()), C.c_void_p(out2.data_ptr()), C.c_void_p(nz2.data_ptr()),
            C.c_void_p(st2.data_ptr()), stream)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(nz, nz2) and torch.equal(st, st2), name
    print(f"{name}: resident key ok", flush=True)


def decode_sets():
    for name in sorted(SETS):
        moduli, l = SETS[name]
        p = P.PvwParametersBuilder().set_parties(3).set_dimension(4).set_l(l).set_moduli(moduli).build()
        noisy = _rns(checked_cases(M.Params(3, 4, l, moduli)), moduli)
        same(P.decode_scalar_pvw_checked(p, noisy), P.decode_scalar_pvw_checked_host(p, noisy), f"decode {name}")
    print("decode sets ok", flush=True)


def tuning_forms():
    prev = _ffi.select("tuning")
    try:
        for name in ("example128_l8", "bench5_l16", "smallQ_l8"):
            moduli, l = SETS[name]
            p = P.PvwParametersBuilder().set_parties(3).set_dimension(4).set_l(l).set_moduli(moduli).build()
            noisy = _rns(checked_cases(M.Params(3, 4, l, moduli))[::3], moduli)
            want = P.decode_scalar_pvw_checked_host(p, noisy)
            for env in ("PVW_DECODE_SMALL", "PVW_DECODE_VARIANT"):
                os.environ[env] = "0" if env == "PVW_DECODE_SMALL" else "1"
                try:
                    same(P.decode_scalar_pvw_checked(p, noisy), want, f"tuning {env} {name}")
                finally:
                    del os.environ[env]
    finally:
        _ffi.select(prev)
    print("tuning forms ok", flush=True)


def main():
    assert torch.cuda.is_available()
    decode_sets()
    p, gpk, parties, cts, scal = honest("bench5 l8", M.bench_moduli(5), 8, 32, 32)
    tampered(p, parties, cts, "bench5 l8")
    many(p, parties, cts, "bench5 l8")
    resident_key(p, parties, cts, "bench5 l8")
    nz, _ = api._secret_residue(p)
    assert nz == 0, nz
    honest("test3 l16", TEST_MODULI, 16, 24, 16)
    honest("smallQ l8", TEST_MODULI[:2], 8, 24, 8, bounds=(1, 3))
    p2, _, parties2, cts2, _ = honest("128-bit l8", EXAMPLE_MODULI, 8, 24, 64, bounds=(1, 1172385))
    tampered(p2, parties2, cts2, "128-bit l8")
    tuning_forms()
    print("CHECKED_DECRYPT_OK", flush=True)


if __name__ == "__main__":
    main()

"""pvw_decrypt_all[_device]: every party of a range decrypts its share from every dealer in one call (examples/pvw.rs:138-170,
tests/crypto.rs:284-287, examples/pvw_valid_dec.rs:201-209).  The contract: out[p][d] is the word pvw_decrypt_batch returns
for party p's key and column on the same input words -- on ragged geometries, on both sides of the party-count dispatch,
on unreduced and extreme words -- plus the oracle on uniform residues, the dealt-share round trip, key hygiene, repeats,
and the full config-3 size."""
import ctypes as C

import numpy as np
import pytest

import pvw_model as M
import pvw_oracle as O
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import EXAMPLE_MODULI, SEED, TEST_MODULI, primes_1mod, rns_to_ring

pytestmark = pytest.mark.gpu


class _Hip:
    """the few HIP runtime calls the device-pointer tests need (device buffers, a stream of the caller's own)"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")

    def _ok(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def malloc(self, nbytes):
        p = C.c_void_p()
        self._ok(self.L.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))))
        return p.value

    def free(self, p):
        self._ok(self.L.hipFree(C.c_void_p(p)))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        self._ok(self.L.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1))
        return p

    def download(self, p, shape, dtype=np.uint64, offset=0):
        a = np.empty(shape, dtype=dtype)
        self._ok(self.L.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(p + offset), C.c_size_t(a.nbytes), 2))
        return a

    def stream(self):
        s = C.c_void_p()
        self._ok(self.L.hipStreamCreate(C.byref(s)))
        return s

    def sync(self, s=None):
        self._ok(self.L.hipStreamSynchronize(s) if s is not None else self.L.hipDeviceSynchronize())


def _params(n, k, l, moduli):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()


def _random_inputs(p, lo, hi, D, seed):
    rng = np.random.default_rng(seed)
    q = np.array(p.moduli(), dtype=np.uint64)[:, None]
    sk = rng.integers(-2, 3, size=(hi - lo, p.k, p.l), dtype=np.int64)
    c1 = (rng.integers(0, 1 << 63, size=(D, p.k, p.L, p.l), dtype=np.uint64) % q).astype(np.uint64)
    c2 = (rng.integers(0, 1 << 63, size=(D, p.n, p.L, p.l), dtype=np.uint64) % q).astype(np.uint64)
    return sk, c1, c2


def _all(p, lo, hi, sk, c1, c2, repr=P.REPR_NTT):
    out = np.zeros((hi - lo, c1.shape[0]), dtype=np.uint64)
    # the contiguous copies are held in locals: a temporary's buffer would be freed before the call reads it
    sk, c1, c2 = np.ascontiguousarray(sk), np.ascontiguousarray(c1), np.ascontiguousarray(c2)
    p._call("pvw_decrypt_all", lo, hi, sk.ctypes.data, c1.ctypes.data, c2.ctypes.data, c1.shape[0], repr, out.ctypes.data)
    return out


def _per_party(p, sk_p, c1, c2col, repr=P.REPR_NTT, noisy=False):
    out = np.zeros(c1.shape[0], dtype=np.uint64)
    nz = np.zeros((c1.shape[0], p.L, p.l), dtype=np.uint64) if noisy else None
    sk_p, c1, c2col = np.ascontiguousarray(sk_p), np.ascontiguousarray(c1), np.ascontiguousarray(c2col)   # held: see _all
    p._call("pvw_decrypt_batch", sk_p.ctypes.data, c1.ctypes.data, c2col.ctypes.data, c1.shape[0], repr, out.ctypes.data,
            None if nz is None else nz.ctypes.data)
    return (out, nz) if noisy else out


def _check_against_per_party(p, lo, hi, sk, c1, c2, got, parties=None, repr=P.REPR_NTT):
    for i in (range(hi - lo) if parties is None else parties):
        want = _per_party(p, sk[i], c1, c2[:, lo + i], repr)
        assert np.array_equal(got[i], want), f"party {lo + i}: {np.flatnonzero(got[i] != want)[:8]}"


def _residue(p):
    nz, sc = P.api._secret_residue(p)
    return nz, sc


# (n, k, l, moduli, lo, hi, D): l 8..64, L 3 / 4 / 17, k off multiples of 4 and 64, party counts on both sides of the
# dispatch threshold (22) and across the 256-row workgroup edge, dealer counts across the 16 / 128 groupings
GEOMETRIES = [
    (300, 64, 8, M.bench_moduli(17), 3, 260, 129),      # 257 parties from 3, 129 dealers (two groups, the second of one)
    (260, 37, 32, EXAMPLE_MODULI, 1, 256, 300),          # 255 parties, 300 dealers, k = 37
    (20, 6, 16, TEST_MODULI, 0, 5, 17),                  # 5 parties: the per-party side
    (40, 16, 64, primes_1mod(128, 3), 2, 30, 3),         # 28 parties, l = 64 (s-hat through API-layout rows)
    (20, 16, 64, primes_1mod(128, 3), 2, 19, 3),         # 17 parties, l = 64, the per-party side
    (24, 4, 8, TEST_MODULI, 7, 8, 1),                    # one party, one dealer
    (140, 256, 8, M.bench_moduli(17), 0, 130, 128),      # config-3 k, 130 parties, one full group of 128
]


@pytest.mark.parametrize("n,k,l,moduli,lo,hi,D", GEOMETRIES)
def test_equals_the_per_party_path(n, k, l, moduli, lo, hi, D):
    p = _params(n, k, l, moduli)
    sk, c1, c2 = _random_inputs(p, lo, hi, D, seed=n * 1000 + D)
    got = _all(p, lo, hi, sk, c1, c2)
    _check_against_per_party(p, lo, hi, sk, c1, c2, got)
    assert _residue(p)[0] == 0


def test_uniform_residues_against_the_oracle():
    n, k, l, moduli = 40, 12, 8, TEST_MODULI
    p = _params(n, k, l, moduli)
    m = M.Params(n, k, l, moduli)
    orc = O.Oracle(moduli, l)
    lo, hi, D = 2, 22, 5
    sk, c1, c2 = _random_inputs(p, lo, hi, D, seed=7)
    got = _all(p, lo, hi, sk, c1, c2)
    for i in (0, 7, 19):
        noisy = orc.decrypt_noisy(sk[i], c1, c2[:, lo + i])
        want = [M.decode_scalar_pvw(rns_to_ring(noisy[d], moduli), m) for d in range(D)]
        assert [int(v) for v in got[i]] == want


def _system(n, k, l, moduli, seed=SEED):
    p = _params(n, k, l, moduli)
    crs = P.PvwCrs.new_deterministic(p, seed)
    gpk = P.GlobalPublicKey.new(crs)
    parties = [P.Party.new(i, p, seed) for i in range(n)]
    gpk.generate_all_party_keys(parties, seed)
    return p, gpk, parties


def test_dealt_shares_round_trip_and_the_valid_subset():
    n = 40
    p, gpk, parties = _system(n, 16, 8, EXAMPLE_MODULI)
    shares = [[(d * 7919 + j * 104729 + 1) % (1 << 32) for j in range(n)] for d in range(n)]
    cts = P.encrypt_all_party_shares(shares, gpk, SEED)
    res = P.decrypt_all_party_shares(cts, parties)                       # results[recipient][dealer], examples/pvw.rs:157-170
    want = np.array(shares, dtype=np.uint64).T
    assert (res == want).mean() >= 0.99, (res != want).sum()
    for i in (0, 17, n - 1):
        assert list(res[i]) == P.decrypt_party_shares(cts, parties[i].secret_key, i)
    # the valid subset (pvw_valid_dec.rs:162-209): a shuffled selection of dealers, parties [5, 30)
    sel = list(np.random.default_rng(3).permutation(n)[:13])
    sub = P.decrypt_many([cts[d] for d in sel], [pt.secret_key for pt in parties[5:30]], 5)
    assert np.array_equal(sub, res[5:30][:, sel])
    assert _residue(p)[0] == 0


def test_power_basis_input_equals_ntt_input_and_leaves_the_buffers_alone():
    p = _params(50, 24, 16, TEST_MODULI)
    lo, hi, D = 4, 44, 20
    sk, c1, c2 = _random_inputs(p, lo, hi, D, seed=11)
    c1p, c2p = p.ntt_inverse(c1), p.ntt_inverse(c2)
    keep1, keep2 = c1p.copy(), c2p.copy()
    got_pb = _all(p, lo, hi, sk, c1p, c2p, P.REPR_POWER)
    assert np.array_equal(c1p, keep1) and np.array_equal(c2p, keep2)
    assert np.array_equal(got_pb, _all(p, lo, hi, sk, c1, c2))
    _check_against_per_party(p, lo, hi, sk, c1p, c2p, got_pb, parties=(0, 13, 39), repr=P.REPR_POWER)
    # few parties: the per-party side with power-basis input
    got_few = _all(p, lo, lo + 3, sk[:3], c1p, c2p, P.REPR_POWER)
    assert np.array_equal(got_few, got_pb[:3])


@pytest.mark.parametrize("hi", [3, 40])
def test_unreduced_and_extreme_words(hi):
    p = _params(48, 32, 8, EXAMPLE_MODULI)
    lo, D = 0, 24
    sk, c1, c2 = _random_inputs(p, lo, hi, D, seed=hi)
    sk[0, 0, :] = 2                                                   # secret coefficients at the CBD extremes (variance 0.5: +-1 ..)
    sk[1, :, 0] = -2
    q = np.array(p.moduli(), dtype=np.uint64)[:, None]
    c1[0, :5] = 0
    c1[1, :5] = (q - 1)
    c2[2, :] = q - 1
    c2[3, :] = 0
    base = _all(p, lo, hi, sk, c1, c2)
    # c1 words loaded unreduced (w + q where it fits): the inner products reduce them, the result is unchanged
    c1u = c1.copy()
    c1u[4:] += q
    c1u[5, 3:] = np.uint64(0xFFFFFFFFFFFFFFFF)                        # byte-extreme words
    got1 = _all(p, lo, hi, sk, c1u, c2)
    _check_against_per_party(p, lo, hi, sk, c1u, c2, got1, parties=range(min(hi - lo, 6)))
    assert np.array_equal(got1[:, :5], base[:, :5])
    # c2 words loaded unreduced: subtracted as the per-party path subtracts them
    c2u = c2.copy()
    c2u[6:12] += q
    c2u[13, :] = np.uint64(0xFFFFFFFFFFFFFFFF)
    got2 = _all(p, lo, hi, sk, c1, c2u)
    _check_against_per_party(p, lo, hi, sk, c1, c2u, got2, parties=range(min(hi - lo, 6)))
    assert np.array_equal(got2[:, :6], base[:, :6])
    # a word w means w mod q: the modified dealers equal the oracle on the reduced words (and so does the per-party path)
    m = M.Params(48, 32, 8, EXAMPLE_MODULI)
    orc = O.Oracle(EXAMPLE_MODULI, 8)
    for got, c1x, c2x in ((got1, c1u, c2), (got2, c1, c2u)):
        for i in sorted({0, 1, hi - lo - 1}):
            noisy = orc.decrypt_noisy(sk[i], c1x % q, c2x[:, lo + i] % q)
            want = [M.decode_scalar_pvw(rns_to_ring(noisy[d], EXAMPLE_MODULI), m) for d in range(D)]
            assert [int(v) for v in got[i]] == want, f"party {lo + i}"
            assert [int(v) for v in _per_party(p, sk[i], c1x, c2x[:, lo + i])] == want


def _device_variant_body():
    p = _params(200, 64, 8, M.bench_moduli(9))
    lo, hi, D = 10, 190, 40
    sk, c1, c2 = _random_inputs(p, lo, hi, D, seed=5)
    a = _all(p, lo, hi, sk, c1, c2)
    nz, sc = _residue(p)
    assert nz == 0 and sc > 0
    assert np.array_equal(a, _all(p, lo, hi, sk, c1, c2))
    hip = _Hip()
    d_sk, d_c1, d_c2 = hip.upload(sk), hip.upload(c1), hip.upload(c2)
    d_out = hip.malloc((hi - lo) * D * 8)
    stream = hip.stream()
    try:
        for parties in ((lo, hi), (lo, lo + 4)):                      # both sides of the dispatch
            n_p = parties[1] - parties[0]
            p._call("pvw_decrypt_all_device", parties[0], parties[1], d_sk, d_c1, d_c2, D, P.REPR_NTT, d_out, stream)
            hip.sync(stream)
            assert np.array_equal(hip.download(d_out, (n_p, D)), a[:n_p])
            assert _residue(p)[0] == 0
    finally:
        hip.sync()
        for ptr in (d_sk, d_c1, d_c2, d_out):
            hip.free(ptr)
        hip.L.hipStreamDestroy(stream)


def _full_size_body():
    # P = D = 4096 at the config-3 geometry (k = 256, l = 8, 17 limbs): ciphertexts made on the device (keygen, then
    # pvw_encrypt_multi_device), all 16.7 M results against the dealt shares, a seeded sample against the per-party path
    n, k, l = 4096, 256, 8
    moduli = M.bench_moduli(17)
    L = len(moduli)
    p = _params(n, k, l, moduli)
    assert p.verify_correctness_condition()
    crs = P.PvwCrs.new_deterministic(p, SEED)
    P.GlobalPublicKey.new(crs)
    sk = np.zeros((n, k, l), dtype=np.int64)
    p._call("pvw_sample_secret_keys", _ffi_seed(SEED).ctypes.data, 0, n, sk.ctypes.data)
    p._call("pvw_keygen", 0, n, sk.ctypes.data, None, _ffi_seed(SEED).ctypes.data)
    scalars = np.random.default_rng(42).integers(0, 1 << 32, size=(n, n), dtype=np.uint64)
    seeds = np.frombuffer(b"".join(bytes([d & 0xFF, d >> 8]) * 16 for d in range(n)), dtype=np.uint8).copy()
    hip = _Hip()
    P_w = L * l
    d_sc, d_sk = hip.upload(scalars), hip.upload(sk)
    d_c1, d_c2 = hip.malloc(n * k * P_w * 8), hip.malloc(n * n * P_w * 8)
    d_out = hip.malloc(n * n * 8)
    try:
        p._call("pvw_encrypt_multi_device", d_sc, n, n, seeds.ctypes.data, d_c1, d_c2, P.REPR_NTT, None)
        p._call("pvw_decrypt_all_device", 0, n, d_sk, d_c1, d_c2, n, P.REPR_NTT, d_out, None)
        p.synchronize()
        out = hip.download(d_out, (n, n))
        assert (out == scalars.T).mean() > 0.9999, int((out != scalars.T).sum())
        c1 = hip.download(d_c1, (n, k, L, l))
        for i in np.random.default_rng(9).choice(n, 3, replace=False):
            c2col = np.stack([hip.download(d_c2, (L, l), offset=(d * n + int(i)) * P_w * 8) for d in range(n)])
            assert np.array_equal(out[i], _per_party(p, sk[i], c1, c2col))
        assert _residue(p)[0] == 0
    finally:
        hip.sync()
        for ptr in (d_sc, d_sk, d_c1, d_c2, d_out):
            hip.free(ptr)


def _in_fresh_process(body, timeout):
    # device buffers come from the HIP runtime the library itself loaded; a process that has imported a framework with a
    # runtime of its own (as other test modules do) is not the place for that, so these run in a child of their own
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = {[here, os.path.dirname(here), os.path.join(os.path.dirname(here), 'oracle')]!r}; " \
           f"import test_gpu_decrypt_all as t; t.{body}(); print('BODY_OK')"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "BODY_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_key_hygiene_repeats_and_the_device_variant_on_a_caller_stream():
    _in_fresh_process("_device_variant_body", 300)


def test_full_size_config3():
    _in_fresh_process("_full_size_body", 900)


def _ffi_seed(seed):
    return np.frombuffer(seed, dtype=np.uint8).copy()


def test_cpp_mirror_round_trip():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "build", "decrypt_all_cpp_gpu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(root, "pvw_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(root, "tests", "cpp", "decrypt_all.cpp"), "-o", exe,
                           "-L" + libdir, "-lpvw_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DECRYPT_ALL_CPP_OK" in out.stdout, out.stdout + out.stderr

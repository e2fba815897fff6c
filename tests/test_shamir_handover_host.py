"""The one-word handover with weights from a mask, the CPU half: pvw_shamir_handover_weights_host against Lagrange
by pow(x, -1, p) and against pvw_shamir_lagrange_weights_at over the compacted holders, the mask helper against a Python loop,
the whole handover in integers (old shares re-dealt by pvw_shamir_shares_host, integer combinations under the weight rows, t + 1
new shares give the old secret back; the same for a packed old sharing), every refusal at every entry point with nothing
written, the kernels' masked sequence as a stand-alone program under sanitizers, the names and the mirrors.  No device is used."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from test_shamir_host import P62, ROOT, params, primes_for, seeds_for

LIBDIR = os.path.join(ROOT, "pvw_rs_amd")
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")
NEW = ["pvw_shamir_handover_weights_host", "pvw_shamir_handover_weights_device", "pvw_shamir_valid_mask_host",
       "pvw_shamir_valid_mask_device", "pvw_decrypt_all_handover", "pvw_decrypt_all_handover_device"]
MIRRORS = ["shamir_handover_weights", "shamir_valid_mask", "decrypt_all_party_handover"]
SIZES = [1, 2, 6, 65, 257]


def test_exports_of_both_libraries_the_header_and_the_rust_block():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "pvw-hip-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert name in _ffi._SIGNATURES and ("PVW_API int32_t " + name + "(") in header and ("pub fn " + name + "(") in sys_rs, name
        for lib in ("libpvw_hip.so", "libpvw_hip_tuning.so"):
            assert hasattr(C.CDLL(os.path.join(LIBDIR, lib)), name), (lib, name)


def test_mirrors():
    hpp = open(os.path.join(ROOT, "pvw_rs_amd", "host", "pvw.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "pvw", "src", "crypto.rs")).read()
    for name in MIRRORS:
        assert name in P.__all__ and callable(getattr(P, name)), name
        assert ("inline" in hpp and " " + name + "(" in hpp) and "pub fn " + name + "(" in rs, name


def centre(w, p):
    return w - p if w > p // 2 else w


def weights_ref(p, indices, valid, targets):
    """rows [T][D] by Lagrange with pow(x, -1, p); targets None is the point 0"""
    D = len(indices)
    vs = [d for d in range(D) if valid is None or valid[d]]
    pts = [0] if targets is None else [(t + 1) % p for t in targets]
    rows = []
    for z in pts:
        row = [0] * D
        for d in vs:
            num = den = 1
            for e in vs:
                if e != d:
                    num = num * (z - indices[e] - 1) % p
                    den = den * (indices[d] - indices[e]) % p
            row[d] = centre(num * pow(den, -1, p) % p, p)
        rows.append(row)
    return rows


def masks_for(D):
    """none, one holder masked, one holder valid, all masked"""
    out = [None, [int(d != D // 2) for d in range(D)], [int(d == D - 1) for d in range(D)], [0] * D]
    return out if D > 1 else [None, [0]]


def indices_for(D, p, rng):
    """distinct, below p - 1, the largest one included"""
    pool = range(p - 1) if p - 1 <= 4 * D else None
    idx = rng.sample(pool, D - 1) if pool is not None else list({rng.randrange(p - 2) for _ in range(3 * D)})[:D - 1]
    idx = [i for i in idx if i != p - 2][:D - 1]
    while len(idx) < D - 1:
        c = rng.randrange(p - 2)
        if c not in idx:
            idx.append(c)
    idx.insert(rng.randrange(D), p - 2)
    return idx


def targets_for(p, idx, valid, rng):
    """T = 3: the point 0 or -m, a target on a valid holder (where there is one) and one on a masked holder (likewise)"""
    D = len(idx)
    on = [d for d in range(D) if valid is None or valid[d]]
    off = [d for d in range(D) if valid is not None and not valid[d]]
    return [p - 1 - rng.choice([0, 1, 2]) if p > D + 3 else p - 1, idx[on[-1]] if on else p - 1, idx[off[0]] if off else p - 1 - 1 * (p > D + 2)]


@pytest.mark.parametrize("D", SIZES)
def test_weights_against_lagrange_and_the_compacted_host_routine(D):
    rng = random.Random(D)
    grid = primes_for(D + 3)
    assert P62 in grid and len(grid) == 5
    for p in grid:
        idx = indices_for(D, p, rng)
        assert max(idx) == p - 2 and len(set(idx)) == D
        for valid in masks_for(D):
            for targets in (None, targets_for(p, idx, valid, rng)):
                got, count = P.shamir_handover_weights(None, idx, p, valid, targets, host=True)
                vs = [d for d in range(D) if valid is None or valid[d]]
                assert count == len(vs)
                assert got.dtype == np.int64 and got.shape == (1 if targets is None else 3, D)
                assert got.tolist() == weights_ref(p, idx, valid, targets), (p, D, valid, targets)
                want = [[0] * D for _ in got]
                if vs:                                                 # bit for bit the compacted routine, scattered back
                    comp = P.shamir_lagrange_weights_at([idx[d] for d in vs], [p - 1] if targets is None else targets, p)
                    for j, row in enumerate(comp):
                        for d, w in zip(vs, row):
                            want[j][d] = w
                assert got.tolist() == want, (p, D, valid, targets)
                assert all(-(p // 2) <= w <= p // 2 for row in got.tolist() for w in row)
                if targets is not None and vs:                         # on a valid holder: its unit vector, said by the routine itself
                    assert got[1].tolist() == [int(d == vs[-1]) for d in range(D)]
                if not vs:
                    assert not got.any()


def test_centring_at_the_largest_prime():
    """p just below 2^62: a residue above p / 2 must come out negative, and both signs occur"""
    idx = [0, 1, 2, P62 - 2]
    got, _ = P.shamir_handover_weights(None, idx, P62, [1, 1, 0, 1], [P62 - 1, 7], host=True)
    flat = [w for row in got.tolist() for w in row]
    assert any(w < 0 for w in flat) and any(w > 0 for w in flat) and all(abs(w) <= P62 // 2 for w in flat)
    assert got.tolist() == weights_ref(P62, idx, [1, 1, 0, 1], [P62 - 1, 7])


def mask_ref(status, noise, bits, bound):
    rows, count = (status if status is not None else noise).shape
    out = []
    for c in range(count):
        bad = False
        for r in range(rows):
            bad = bad or (status is not None and int(status[r, c]) & bits != 0) or (noise is not None and int(noise[r, c]) > bound)
        out.append(int(not bad))
    return out


def test_mask_helper_against_a_python_loop():
    rng = random.Random(5)
    lib = _ffi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for rows, count in ((1, 1), (1, 70), (3, 6), (12, 65)):
        status = np.array([[rng.choice([0, 0, 0, 1, 2, 4, 6]) for _ in range(count)] for _ in range(rows)], dtype=np.uint32)
        noise = np.array([[rng.choice([0, 5, 9, 10, 11, 2**64 - 1]) for _ in range(count)] for _ in range(rows)], dtype=np.uint64)
        for st, nz in ((status, noise), (status, None), (None, noise)):
            for bits, bound in ((0xFFFFFFFF, 10), (2, 2**64 - 1), (5, 9)):
                want = mask_ref(st, nz, bits, bound)
                got, num = P.shamir_valid_mask(st, nz, status_bits=bits, noise_bound=bound, host=True)
                assert got.tolist() == want and num == sum(want), (rows, count, bits, bound)
                # the other stride pair: the same report stored [count][rows], read with strides (1, rows)
                stT = None if st is None else np.ascontiguousarray(st.T)
                nzT = None if nz is None else np.ascontiguousarray(nz.T)
                out, n2 = np.full(count, 7, dtype=np.uint8), C.c_uint32()
                assert lib.pvw_shamir_valid_mask_host(ptr(stT), ptr(nzT), bits, bound, count, rows, 1, rows, ptr(out), C.byref(n2)) == 0
                assert out.tolist() == want and n2.value == sum(want)
                assert lib.pvw_shamir_valid_mask_host(ptr(stT), ptr(nzT), bits, bound, count, rows, 1, rows, ptr(out), None) == 0
    # col_err as status: the columns with a wrong share are the masked holders
    col_err = np.array([0, 3, 0, 0, 1, 0], dtype=np.uint32)
    got, num = P.shamir_valid_mask(col_err, host=True)
    assert got.tolist() == [1, 0, 1, 1, 0, 1] and num == 4


def poly_shares(p, coeffs, idx):
    return [sum(c * pow(i + 1, e, p) for e, c in enumerate(coeffs)) % p for i in idx]


@pytest.mark.parametrize("p", [65537, P62], ids=lambda p: f"{p.bit_length()}bit")
def test_handover_in_integers(p):
    """the old holders re-deal their shares of a degree-2 sharing; integer combinations under the weight row give every new
    party sum_d lambda_d f_d(j + 1), and t + 1 of those give the old secret back"""
    n, t = 12, 2
    rng = random.Random(p & 0xFF)
    old = [rng.randrange(p) for _ in range(3)]
    idx, valid = [0, 5, 2, 7, 3, 9], [1, 0, 1, 1, 1, 1]
    D = len(idx)
    old_shares = poly_shares(p, old, idx)
    old_shares[1] = (old_shares[1] + 1) % p                             # the masked holder's share is wrong: it must not matter
    redeal = P.shamir_shares(params(n), old_shares, t, p, seeds=seeds_for(D, tag=3), host=True).tolist()      # [D][n]
    rows, count = P.shamir_handover_weights(None, idx, p, valid, None, host=True)
    assert count == 5 and rows.shape == (1, D)
    lam = rows[0].tolist()
    new = [sum(lam[d] * redeal[d][j] for d in range(D)) % p for j in range(n)]
    lam_py = weights_ref(p, idx, valid, None)[0]
    assert new == [sum(lam_py[d] * redeal[d][j] for d in range(D)) % p for j in range(n)]
    for _ in range(3):
        pick = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct(pick, [new[j] for j in pick], p) == old[0]


def test_handover_of_a_packed_old_sharing_in_integers():
    p, n, t, K, told, nold = P62, 9, 2, 3, 2, 7
    rng = random.Random(3)
    secrets = [rng.randrange(p) for _ in range(K)]
    old = P.shamir_shares_packed(params(nold), [secrets], told, p, seeds=seeds_for(1), host=True)[0].tolist()    # degree told + K - 1 = 4
    idx, valid = [0, 1, 3, 4, 5, 6], [1, 1, 1, 0, 1, 1]                   # five valid holders determine degree 4
    D = len(idx)
    redeal = P.shamir_shares(params(n), [old[i] for i in idx], t, p, seeds=seeds_for(D, tag=9), host=True).tolist()
    rows, count = P.shamir_handover_weights(None, idx, p, valid, [p - 1 - m for m in range(K)], host=True)
    assert count == 5 and rows.shape == (K, D)
    rows = rows.tolist()
    new = [[sum(rows[m][d] * redeal[d][j] for d in range(D)) % p for m in range(K)] for j in range(n)]
    for m in range(K):
        pick = rng.sample(range(n), t + 1)
        assert P.shamir_reconstruct(pick, [new[j][m] for j in pick], p) == secrets[m]


def test_refusals_of_every_entry_point():
    lib = _ffi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    pr = params(12)
    p = 65537
    idx = np.array([0, 1, 2], dtype=np.uint64)
    dup = np.array([0, 1, 1], dtype=np.uint64)
    far = np.array([0, 1, p - 1], dtype=np.uint64)
    m110 = np.array([1, 1, 0], dtype=np.uint8)
    tg = np.array([p - 1, 4], dtype=np.uint64)
    tbad = np.array([p - 1, p], dtype=np.uint64)
    out = np.full(64, 77, dtype=np.int64)
    cnt = C.c_uint32(99)
    for fn, head, tail in ((lib.pvw_shamir_handover_weights_host, (), ()), (lib.pvw_shamir_handover_weights_device, (pr._h,), (None,))):
        bad = [
            (p, None, None, 3, None, 1, ptr(out)),
            (p, ptr(idx), None, 3, None, 1, None),
            (p, ptr(idx), None, 0, None, 1, ptr(out)),                   # no holders
            (p, ptr(idx), None, 3, ptr(tg), 0, ptr(out)),                # T = 0
            (p, ptr(idx), None, 3, None, 2, ptr(out)),                   # NULL targets with T != 1
            (p - 1, ptr(idx), None, 3, None, 1, ptr(out)),               # not prime
            (1 << 62, ptr(idx), None, 3, None, 1, ptr(out)),             # not below 2^62
            (p, ptr(dup), None, 3, None, 1, ptr(out)),                   # a duplicate
            (p, ptr(dup), ptr(m110), 3, None, 1, ptr(out)),              # ... also where the mask hides it
            (p, ptr(far), None, 3, None, 1, ptr(out)),                   # an index >= p - 1
            (p, ptr(far), ptr(m110), 3, None, 1, ptr(out)),              # ... also where the mask hides it
            (p, ptr(idx), None, 3, ptr(tbad), 2, ptr(out)),              # a target >= p
        ]
        for args in bad:
            assert fn(*head, *args, C.byref(cnt), *tail) == 1, (fn.__name__, args)
            assert (out == 77).all() and cnt.value == 99
    assert lib.pvw_shamir_handover_weights_device(None, p, ptr(idx), None, 3, None, 1, ptr(out), None, None) == 1
    # the device's bounds, refused before an array of that length is looked at
    assert lib.pvw_shamir_handover_weights_device(pr._h, p, ptr(idx), None, 1 << 32, None, 1, ptr(out), None, None) == 1
    assert lib.pvw_shamir_handover_weights_device(pr._h, p, ptr(idx), None, 3, ptr(tg), 1 << 31, ptr(out), None, None) == 1
    assert (out == 77).all()
    # the mask helper: the rules of pvw_shamir_erasure_mask_*
    st, nz, v = np.zeros(6, np.uint32), np.zeros(6, np.uint64), np.full(6, 9, np.uint8)
    for fn, head, tail in ((lib.pvw_shamir_valid_mask_host, (), ()), (lib.pvw_shamir_valid_mask_device, (pr._h,), (None,))):
        bad = [
            (None, None, 1, 0, 6, 1, 6, 1, ptr(v)),
            (ptr(st), ptr(nz), 1, 0, 6, 1, 6, 1, None),
            (ptr(st), ptr(nz), 1, 0, 0, 1, 6, 1, ptr(v)),
            (ptr(st), ptr(nz), 1, 0, 6, 0, 6, 1, ptr(v)),
            (ptr(st), ptr(nz), 1, 0, 6, 1, 0, 1, ptr(v)),
            (ptr(st), ptr(nz), 1, 0, 6, 1, 6, 0, ptr(v)),
        ]
        for args in bad:
            assert fn(*head, *args, C.byref(cnt), *tail) == 1, (fn.__name__, args)
            assert (v == 9).all() and cnt.value == 99
    assert lib.pvw_shamir_valid_mask_device(None, ptr(st), ptr(nz), 1, 0, 6, 1, 6, 1, ptr(v), None, None) == 1
    assert lib.pvw_shamir_valid_mask_device(pr._h, ptr(st), ptr(nz), 1, 0, 1 << 31, 1, 6, 1, ptr(v), None, None) == 1
    assert lib.pvw_shamir_valid_mask_device(pr._h, ptr(st), ptr(nz), 1, 0, 6, 1 << 31, 6, 1, ptr(v), None, None) == 1
    # the handover in one call: every refusal comes before any device work (this machine has no device to reach)
    p17 = P.PvwParametersBuilder().set_parties(12).set_dimension(16).set_l(8).set_moduli(M.bench_moduli(17)).build()
    qwords = (p17.q_total().bit_length() + 63) // 64
    buf = np.full(8, 5, dtype=np.uint64)
    idx6, dup6 = np.arange(6, dtype=np.uint64), np.array([0, 1, 2, 3, 4, 4], dtype=np.uint64)
    none6 = np.zeros(6, dtype=np.uint8)
    for name in ("pvw_decrypt_all_handover", "pvw_decrypt_all_handover_device"):
        fn = getattr(lib, name)
        tail = (None,) if name.endswith("_device") else ()
        #        0      1  2   3         4         5        6  7     8          9     10 11          12        13    14    15    16 17 18
        good = [p17._h, 0, 12, ptr(buf), ptr(buf), ptr(buf), 6, None, ptr(idx6), None, 1, P.REPR_NTT, ptr(buf), None, None, None, p, 0, None]
        for pos, value in ((0, None), (3, None), (4, None), (5, None), (6, 0), (8, None), (8, ptr(dup6)), (10, 0), (10, 2), (12, None),
                           (16, p - 1), (16, 1 << 62), (16, 0), (17, qwords + 1), (17, 1), (1, 12), (2, 13)):
            args = list(good)
            args[pos] = value
            assert fn(*args, *tail) == 1, (name, pos, value)
            assert (buf == 5).all()
        args = list(good)
        args[9], args[10] = ptr(np.array([p], dtype=np.uint64)), 1     # a target >= p
        assert fn(*args, *tail) == 1, name
        args = list(good)
        args[11] = 7                                                    # the many-combinations call's own code for a representation
        assert fn(*args, *tail) == 18, name
    # host buffers with nobody valid: the mirrored call's code, before any device work
    args = list(good)
    args[0], args[7] = p17._h, ptr(none6)
    assert lib.pvw_decrypt_all_handover(*args[:19]) == 17
    assert "No valid dealer" in _ffi.last_error(lib)


def build_kernel_sequence():
    """tests/cpp/shamir_handover.cpp under the address and undefined-behaviour sanitizers, as a program of its own"""
    exe = os.path.join(ROOT, "build", "shamir_handover")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_handover.cpp"), "-o", exe])
    return exe


def test_kernel_sequence_against_the_host_routine_under_sanitizers():
    """tests/cpp/shamir_handover.cpp restates the kernels' masked sequence (ballots of 64 mask bytes, the masked column weights,
    the masked scale and coinciding column, the Cauchy entries eight to an inversion, the weights kernel, the count) over
    pvw_arith.h, built with the address and undefined-behaviour sanitizers as a program of its own; what it prints is compared
    here with pvw_shamir_handover_weights_host.  Nothing sanitized is loaded into Python."""
    exe = build_kernel_sequence()
    rng = random.Random(11)
    for D in (1, 7, 9, 65, 130, 257):
        for p in primes_for(D + 3):
            idx = indices_for(D, p, rng)
            masks = masks_for(D) + ([[int(d >= 64) for d in range(D)]] if D > 64 else [])     # only holders beyond lane 63
            for valid in masks:
                targets = targets_for(p, idx, valid, rng)
                out = subprocess.run([exe, str(p), "-" if valid is None else "".join(map(str, valid)), ",".join(map(str, idx)),
                                      ",".join(map(str, targets))], capture_output=True, text=True, timeout=120)
                assert out.returncode == 0 and "SHAMIR_HANDOVER_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
                lines = out.stdout.splitlines()
                want, count = P.shamir_handover_weights(None, idx, p, valid, targets, host=True)
                assert lines[0] == f"C {count}", (D, p, valid)
                assert [int(x) for x in lines[1].split()[1:]] == want.reshape(-1).tolist(), (D, p, valid)


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "shamir_handover_mirror.cpp")
CPP_EXE = os.path.join(ROOT, "build", "shamir_handover_cpp")


def test_cpp_mirror_on_the_host():
    os.makedirs(os.path.dirname(CPP_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", CPP_SRC, "-o", CPP_EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([CPP_EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_HANDOVER_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

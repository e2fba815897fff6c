"""pvw_decrypt_all / pvw_decrypt_all_device (every party decrypts its share from every dealer, examples/pvw.rs:138-170)
on the host side: the symbols exist in both builds, argument errors come back with their codes before any device work,
the Python mirror raises the reference's messages (decryption.rs:286-305) first, and the C++ mirror compiles.  No device
compute here; the results are checked in tests/test_gpu_decrypt_all.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import TEST_MODULI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS, INVALID_FORMAT, INTERNAL = 1, 18, 19


def _params(n=6, k=4, l=8):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(TEST_MODULI).build()


def _buffers(p, parties, dealers):
    sk = np.zeros((parties, p.k, p.l), dtype=np.int64)
    c1 = np.zeros((dealers, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((dealers, p.n, p.L, p.l), dtype=np.uint64)
    out = np.zeros((parties, dealers), dtype=np.uint64)
    return sk, c1, c2, out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _rc(lib, name, p, lo, hi, sk, c1, c2, D, repr, out):
    args = [p._h, lo, hi, sk, c1, c2, D, repr, out] + ([None] if name.endswith("_device") else [])
    return getattr(lib, name)(*args)


def test_both_libraries_export_the_entry_points():
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        assert hasattr(lib, "pvw_decrypt_all") and hasattr(lib, "pvw_decrypt_all_device")


def test_the_shipped_library_has_no_dispatch_switch():
    s = subprocess.run(["strings", "-a", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "PVW_DECRYPT_ALL_MIN_PARTIES" not in s
    s = subprocess.run(["strings", "-a", _ffi.LIB_TUNING_PATH], capture_output=True, text=True, check=True).stdout
    assert "PVW_DECRYPT_ALL_MIN_PARTIES" in s


@pytest.mark.parametrize("name", ["pvw_decrypt_all", "pvw_decrypt_all_device"])
def test_argument_errors_come_before_the_device(name):
    lib = _ffi.lib()
    p = _params()
    sk, c1, c2, out = _buffers(p, 2, 3)
    cases = [
        ((1, 3, None, _ptr(c1), _ptr(c2), 3, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "NULL argument"),
        ((1, 3, _ptr(sk), None, _ptr(c2), 3, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "NULL argument"),
        ((1, 3, _ptr(sk), _ptr(c1), None, 3, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "NULL argument"),
        ((1, 3, _ptr(sk), _ptr(c1), _ptr(c2), 3, P.REPR_NTT, None), INVALID_PARAMETERS, "NULL argument"),
        ((1, 3, _ptr(sk), _ptr(c1), _ptr(c2), 0, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "No ciphertexts provided"),
        ((3, 3, _ptr(sk), _ptr(c1), _ptr(c2), 3, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "empty party range"),
        ((4, 3, _ptr(sk), _ptr(c1), _ptr(c2), 3, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "party_lo > party_hi"),
        ((5, 7, _ptr(sk), _ptr(c1), _ptr(c2), 3, P.REPR_NTT, _ptr(out)), INVALID_PARAMETERS, "Party index 6 exceeds maximum 5"),
        ((1, 3, _ptr(sk), _ptr(c1), _ptr(c2), 3, 7, _ptr(out)), INVALID_FORMAT, "unknown representation"),
    ]
    for (lo, hi, a_sk, a_c1, a_c2, D, repr, a_out), code, msg in cases:
        rc = _rc(lib, name, p, lo, hi, a_sk, a_c1, a_c2, D, repr, a_out)
        assert rc == code, (lo, hi, D, repr, rc, _ffi.last_error())
        assert msg in _ffi.last_error()
    assert not out.any()


@pytest.mark.skipif(P.device_available(), reason="a device is present: the call runs (tests/test_gpu_decrypt_all.py)")
@pytest.mark.parametrize("name", ["pvw_decrypt_all", "pvw_decrypt_all_device"])
def test_valid_arguments_without_a_device_fail_loudly(name):
    lib = _ffi.lib()
    p = _params()
    sk, c1, c2, out = _buffers(p, 2, 3)
    rc = _rc(lib, name, p, 1, 3, _ptr(sk), _ptr(c1), _ptr(c2), 3, P.REPR_NTT, _ptr(out))
    assert rc == INTERNAL and "no CPU fallback" in _ffi.last_error()


def _cts(p, D):
    return [P.PvwCiphertext(np.zeros((p.k, p.L, p.l), np.uint64), np.zeros((p.n, p.L, p.l), np.uint64), p, P.REPR_NTT)
            for _ in range(D)]


def test_python_mirror_checks_before_the_device():
    p = _params()
    parties = [P.Party(i, P.SecretKey(p, np.zeros((p.k, p.l), np.int64))) for i in range(p.n)]
    with pytest.raises(P.PvwError, match="No ciphertexts provided"):
        P.decrypt_all_party_shares([], parties)
    with pytest.raises(P.PvwError, match=f"Expected {p.n} ciphertexts, got 5"):
        P.decrypt_all_party_shares(_cts(p, 5), parties)
    with pytest.raises(P.PvwError, match="consecutive"):
        P.decrypt_all_party_shares(_cts(p, p.n), [parties[0], parties[2]])
    with pytest.raises(P.PvwError, match=f"Party index {p.n} exceeds maximum {p.n - 1}"):
        P.decrypt_all_party_shares(_cts(p, p.n), parties[4:] + [P.Party(p.n, parties[0].secret_key)])
    bad = _cts(p, p.n)
    bad[3] = P.PvwCiphertext(np.zeros((p.k - 1, p.L, p.l), np.uint64), bad[3].c2, p, P.REPR_NTT)
    with pytest.raises(P.PvwError, match="Ciphertext 3 invalid"):
        P.decrypt_all_party_shares(bad, parties)
    with pytest.raises(P.PvwError, match="No ciphertexts provided"):
        P.decrypt_many([], [parties[0].secret_key], 0)
    assert P.decrypt_all_party_shares(_cts(p, p.n), []).shape == (0, p.n)


def test_cpp_mirror_compiles_against_the_header():
    exe = os.path.join(ROOT, "build", "decrypt_all_cpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "decrypt_all.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "pvw_rs_amd"), "-lpvw_hip", "-Wl,-rpath," + os.path.join(ROOT, "pvw_rs_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)

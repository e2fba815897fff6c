"""Key generation from a seed on the host side: pvw_keygen_seeded, pvw_sample_secret_keys_device and
pvw_sk_load_seeded are exported by both libraries and declared in the header, their Python names are public, every refusal
that needs no device comes back with its code and text before any device work and with nothing written (sentinel-filled outputs
stay as they were), and the C++ mirror compiles and refuses the same way.  No device compute here; the kernels are checked
bit for bit in tests/test_gpu_keygen_seeded.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import TEST_MODULI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pvw_keygen_seeded", "pvw_sample_secret_keys_device", "pvw_sk_load_seeded"]
INVALID_PARAMETERS, CRS_ERROR, INTERNAL = 1, 6, 19
SRC = os.path.join(ROOT, "tests", "cpp", "keygen_seeded.cpp")
EXE = os.path.join(ROOT, "build", "keygen_seeded_cpp")
LIBDIR = os.path.join(ROOT, "pvw_rs_amd")
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _params(n=6, k=4, l=8):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(TEST_MODULI).build()


def _seed(b):
    return np.full(32, b, dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def refused(lib, rc, code, text):
    assert rc == code and text in _ffi.last_error(lib), (rc, _ffi.last_error(lib))


def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW:
            assert hasattr(lib, name), name
            assert "PVW_API int32_t " + name + "(" in header, name
            assert name in _ffi._SIGNATURES
    # each declaration cites the reference's own setup path
    for name in NEW:
        doc = header[:header.index("PVW_API int32_t " + name + "(")].rsplit("*/", 2)[-2]
        assert "secret_key.rs:45-63" in doc and "public_key.rs:62-79" in doc, name


def test_python_names_are_public():
    assert "sample_secret_keys_device" in P.__all__ and callable(P.sample_secret_keys_device)
    assert {"GlobalPublicKey", "DeviceSecretKey"} <= set(P.__all__)
    assert callable(P.GlobalPublicKey.generate_seeded) and callable(P.DeviceSecretKey.from_seed)


@pytest.mark.parametrize("which", ["default", "tuning"])
def test_keygen_seeded_refuses_before_any_device_work(which):
    prev = _ffi.select(which)
    try:
        lib = _ffi.lib()
        p = _params()                                                  # a context of the library under test
    finally:
        _ffi.select(prev)
    a, b = _seed(1), _seed(2)
    refused(lib, lib.pvw_keygen_seeded(None, 0, 1, _ptr(a), _ptr(b)), INVALID_PARAMETERS, "NULL argument")
    for args in ((0, 1, None, _ptr(b)), (0, 1, _ptr(a), None), (0, 1, None, None)):
        refused(lib, lib.pvw_keygen_seeded(p._h, *args), INVALID_PARAMETERS, "NULL argument")
    refused(lib, lib.pvw_keygen_seeded(p._h, 5, 3, _ptr(a), _ptr(b)), INVALID_PARAMETERS, "party_lo > party_hi")
    refused(lib, lib.pvw_keygen_seeded(p._h, 0, 7, _ptr(a), _ptr(b)), INVALID_PARAMETERS, "Party index 6 exceeds maximum 5")
    # the checks are pvw_keygen's, in its order: the same range through it gives the same text
    sk = np.zeros((7, 4, 8), dtype=np.int64)
    refused(lib, lib.pvw_keygen(p._h, 0, 7, _ptr(sk), None, _ptr(b)), INVALID_PARAMETERS, "Party index 6 exceeds maximum 5")
    n = C.c_uint32(99)
    assert lib.pvw_num_public_keys(p._h, C.byref(n)) == 0 and n.value == 0


def test_stream_index_of_a_drawn_key_must_fit_32_bits():
    lib = _ffi.lib()
    a, b = _seed(1), _seed(2)
    big = _params(n=1 << 22, k=1024)                                   # n k = 2^32
    refused(lib, lib.pvw_keygen_seeded(big._h, 0, 1 << 22, _ptr(a), _ptr(b)), INVALID_PARAMETERS, "below 2^32")
    refused(lib, lib.pvw_keygen_seeded(big._h, (1 << 22) - 1, 1 << 22, _ptr(a), _ptr(b)), INVALID_PARAMETERS, "below 2^32")
    # one party fewer passes the check and reaches the device (or its absence)
    rc = lib.pvw_keygen_seeded(big._h, (1 << 22) - 2, (1 << 22) - 1, _ptr(a), _ptr(b))
    assert rc != INVALID_PARAMETERS and "2^32" not in _ffi.last_error(lib)
    p = _params()                                                      # k = 4: parties up to 2^30 - 1
    h = C.c_void_p(SENTINEL)
    refused(lib, lib.pvw_sample_secret_keys_device(p._h, _ptr(a), 1 << 30, 0, None, None), INVALID_PARAMETERS, "below 2^32")
    refused(lib, lib.pvw_sample_secret_keys_device(p._h, _ptr(a), (1 << 30) - 3, 3, h, None), INVALID_PARAMETERS, "below 2^32")
    refused(lib, lib.pvw_sample_secret_keys_device(p._h, _ptr(a), 0xFFFFFFFF, 0xFFFFFFFF, h, None), INVALID_PARAMETERS, "below 2^32")
    refused(lib, lib.pvw_sk_load_seeded(p._h, _ptr(a), (1 << 30) - 1, C.byref(h)), INVALID_PARAMETERS, "below 2^32")
    assert not h.value                                                 # as pvw_sk_load: no handle on failure


def test_sample_device_and_resident_key_refuse_null_arguments():
    lib = _ffi.lib()
    p = _params()
    a = _seed(3)
    out = np.full((2, 4, 8), SENTINEL, dtype=np.int64)                 # a host buffer standing in: never touched
    refused(lib, lib.pvw_sample_secret_keys_device(None, _ptr(a), 0, 2, _ptr(out), None), INVALID_PARAMETERS, "NULL argument")
    refused(lib, lib.pvw_sample_secret_keys_device(p._h, None, 0, 2, _ptr(out), None), INVALID_PARAMETERS, "NULL argument")
    refused(lib, lib.pvw_sample_secret_keys_device(p._h, _ptr(a), 0, 2, None, None), INVALID_PARAMETERS, "NULL argument")
    assert (out == SENTINEL).all()
    # count == 0 does nothing, with or without a buffer, with or without a device
    assert lib.pvw_sample_secret_keys_device(p._h, _ptr(a), 0, 0, None, None) == 0
    assert lib.pvw_sample_secret_keys_device(p._h, _ptr(a), 3, 0, _ptr(out), None) == 0
    assert (out == SENTINEL).all()
    h = C.c_void_p(SENTINEL)
    refused(lib, lib.pvw_sk_load_seeded(None, _ptr(a), 0, C.byref(h)), INVALID_PARAMETERS, "NULL argument")
    refused(lib, lib.pvw_sk_load_seeded(p._h, None, 0, C.byref(h)), INVALID_PARAMETERS, "NULL argument")
    assert h.value == SENTINEL
    refused(lib, lib.pvw_sk_load_seeded(p._h, _ptr(a), 0, None), INVALID_PARAMETERS, "NULL argument")
    # a variance the sampler refuses is refused here as well, before the device is asked for
    bad = P.PvwParametersBuilder().set_parties(6).set_dimension(4).set_l(8).set_moduli(TEST_MODULI).set_secret_variance(0.75).build()
    assert lib.pvw_sample_secret_keys_device(bad._h, _ptr(a), 0, 2, _ptr(out), None) == 2 and (out == SENTINEL).all()


def test_no_crs_is_refused_where_pvw_keygen_refuses_it():
    """pvw_keygen checks the CRS after it has found the device, and so does the seeded form: CrsError on a GPU, the missing device
    named without one -- in both cases nothing is generated"""
    lib = _ffi.lib()
    p = _params()
    a, b = _seed(1), _seed(2)
    rc = lib.pvw_keygen_seeded(p._h, 0, 6, _ptr(a), _ptr(b))
    if P.device_available():
        refused(lib, rc, CRS_ERROR, "CRS not loaded")
    else:
        refused(lib, rc, INTERNAL, "no HIP device available")
    n = C.c_uint32(99)
    assert lib.pvw_num_public_keys(p._h, C.byref(n)) == 0 and n.value == 0


def test_python_mirror_checks_its_arguments():
    p = _params()
    gpk = P.GlobalPublicKey.__new__(P.GlobalPublicKey)
    gpk.params, gpk.crs = p, None
    with pytest.raises(P.PvwError, match="seed must be 32 bytes"):
        gpk.generate_seeded(0, 6, b"short", bytes(32))
    with pytest.raises(P.PvwError, match="party_lo > party_hi"):
        gpk.generate_seeded(4, 2, bytes(32), bytes(32))
    with pytest.raises(P.PvwError, match="seed must be 32 bytes"):
        P.DeviceSecretKey.from_seed(p, b"short", 0)
    with pytest.raises(P.PvwError, match="below 2\\^32"):
        P.DeviceSecretKey.from_seed(p, bytes(32), (1 << 30) - 1)


def _build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", EXE, "-L" + LIBDIR, "-lpvw_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_mirror_compiles_and_refuses_on_the_host():
    """the pvw_host overloads: the program's host half (argument checks) runs everywhere"""
    _build_cpp()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "KEYGEN_SEEDED_CPP_HOST_OK" in out.stdout, out.stdout + out.stderr

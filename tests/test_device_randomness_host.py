"""Device randomness state (pvw_rnd_state, pvw_encrypt_rs*, pvw_encrypt_multi_rs*) on the host side: the symbols exist in
both builds, pvw_rnd_call_seed is the ChaCha8 block the header defines, argument errors come back before any device work,
and the Python, C++ and Rust mirrors are there.  No device compute here; the encrypts are checked in
tests/test_gpu_device_randomness.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
from _util import TEST_MODULI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_PARAMETERS = 1
NEW_SYMBOLS = ["pvw_rnd_state_create", "pvw_rnd_state_counter", "pvw_rnd_state_set_counter", "pvw_rnd_state_free",
               "pvw_rnd_call_seed", "pvw_encrypt_rs", "pvw_encrypt_rs_device", "pvw_encrypt_multi_rs",
               "pvw_encrypt_multi_rs_device", "pvw_selftest_rnd_free_residue"]


def _params(n=6, k=4, l=8):
    return P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(TEST_MODULI).build()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_both_libraries_export_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "pvw_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"PVW_API int32_t " + name + r"\(", header), name
    for lib in (_ffi.lib(), _ffi.tuning_lib()):
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name
    assert "PVW_DOM_CALL = 8" in header and P.DOM_CALL == 8


def _model_call_seed(seed: bytes, c: int) -> bytes:
    words = M.chacha_block(list(struct.unpack("<8I", seed)), c, 8 << 32)[:8]          # stream id (PVW_DOM_CALL << 32) | 0
    return struct.pack("<8I", *words)


@pytest.mark.parametrize("c", [0, 1, 2, 7, 1000, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 0x0123456789ABCDEF, (1 << 64) - 2,
                               (1 << 64) - 1])
def test_call_seed_is_the_chacha8_block(c):
    for seed in (bytes(32), bytes(range(32)), bytes([0xFF]) * 32, bytes(range(101, 133))):
        want = _model_call_seed(seed, c)
        out = np.zeros(32, dtype=np.uint8)
        assert _ffi.lib().pvw_rnd_call_seed(_ptr(np.frombuffer(seed, np.uint8).copy()), c, _ptr(out)) == 0
        assert out.tobytes() == want
        assert P.DeviceRandomness.call_seed(seed, c) == want


def test_call_seeds_differ_from_the_seed_and_from_each_other():
    seed = bytes(range(32))
    got = {P.DeviceRandomness.call_seed(seed, c) for c in range(64)}
    assert len(got) == 64 and seed not in got


def test_call_seed_argument_errors():
    lib = _ffi.lib()
    out = np.zeros(32, dtype=np.uint8)
    assert lib.pvw_rnd_call_seed(None, 0, _ptr(out)) == INVALID_PARAMETERS
    assert lib.pvw_rnd_call_seed(_ptr(out), 0, None) == INVALID_PARAMETERS
    with pytest.raises(P.PvwError, match="32 bytes"):
        P.DeviceRandomness.call_seed(bytes(31), 0)


def test_state_argument_errors_come_before_the_device():
    lib = _ffi.lib()
    p = _params()
    v = C.c_uint64(0)
    h = C.c_void_p()
    seed = np.zeros(32, dtype=np.uint8)
    assert lib.pvw_rnd_state_create(None, _ptr(seed), 0, C.byref(h)) == INVALID_PARAMETERS
    assert lib.pvw_rnd_state_create(p._h, None, 0, C.byref(h)) == INVALID_PARAMETERS
    assert lib.pvw_rnd_state_create(p._h, _ptr(seed), 0, None) == INVALID_PARAMETERS
    assert lib.pvw_rnd_state_counter(None, None, C.byref(v)) == INVALID_PARAMETERS
    assert lib.pvw_rnd_state_set_counter(None, 3, None) == INVALID_PARAMETERS
    assert lib.pvw_rnd_state_free(None) == 0
    assert lib.pvw_selftest_rnd_free_residue(None) == INVALID_PARAMETERS


@pytest.mark.parametrize("device", [False, True])
def test_encrypt_argument_errors_come_before_the_device(device):
    lib = _ffi.lib()
    p = _params()
    n, D = p.n, 3
    sc = np.zeros((D, n), dtype=np.uint64)
    c1 = np.zeros((D, p.k, p.L, p.l), dtype=np.uint64)
    c2 = np.zeros((D, n, p.L, p.l), dtype=np.uint64)
    # an opaque stand-in handle: the calls below must fail on their other arguments without reading it
    fake = np.zeros(8, dtype=np.uint64)
    tail = [None] if device else []
    single = lib.pvw_encrypt_rs_device if device else lib.pvw_encrypt_rs
    multi = lib.pvw_encrypt_multi_rs_device if device else lib.pvw_encrypt_multi_rs
    cases = [
        (single, (p._h, _ptr(sc), n, None, _ptr(c1), _ptr(c2), P.REPR_NTT), "NULL argument"),
        (single, (p._h, _ptr(sc), n - 1, _ptr(fake), _ptr(c1), _ptr(c2), P.REPR_NTT), f"Must provide exactly n={n} scalars, got {n - 1}"),
        (single, (p._h, _ptr(sc), n, _ptr(fake), _ptr(c1), _ptr(c2), P.REPR_NTT), "Global public key is not complete"),
        (multi, (p._h, _ptr(sc), D, n, None, _ptr(c1), _ptr(c2), P.REPR_NTT), "NULL argument"),
        (multi, (p._h, _ptr(sc), 0, n, _ptr(fake), _ptr(c1), _ptr(c2), P.REPR_NTT), "no dealers"),
        (multi, (p._h, _ptr(sc), D, n + 1, _ptr(fake), _ptr(c1), _ptr(c2), P.REPR_NTT), f"Dealer provided {n + 1} shares but needs {n}"),
        (multi, (p._h, _ptr(sc), D, n, _ptr(fake), _ptr(c1), _ptr(c2), P.REPR_NTT), "Global public key is not complete"),
    ]
    for fn, args, msg in cases:
        assert fn(*(list(args) + tail)) == INVALID_PARAMETERS, (args, _ffi.last_error())
        assert msg in _ffi.last_error(), (msg, _ffi.last_error())
    assert not c1.any() and not c2.any()


@pytest.mark.skipif(P.device_available(), reason="a device is present: the state is created (tests/test_gpu_device_randomness.py)")
def test_creating_a_state_without_a_device_fails_loudly():
    with pytest.raises(P.PvwError, match="no CPU fallback"):
        P.DeviceRandomness(_params(), bytes(32))


def test_python_mirror_checks_before_the_device():
    p = _params()
    gpk = P.GlobalPublicKey(P.PvwCrs(p))
    st = P.DeviceRandomness.__new__(P.DeviceRandomness)       # a handle that was never created
    st.params, st._lib, st._h = p, p._lib, None
    with pytest.raises(P.PvwError, match="either a seed"):
        P.encrypt([0] * p.n, gpk, bytes(32), randomness=st)
    with pytest.raises(P.PvwError, match="has been freed"):
        P.encrypt([0] * p.n, gpk, randomness=st)
    with pytest.raises(P.PvwError, match="must be a DeviceRandomness"):
        P.encrypt([0] * p.n, gpk, randomness=bytes(32))
    with pytest.raises(P.PvwError, match="either a seed"):
        P.encrypt_broadcast(1, gpk, bytes(32), randomness=st)
    with pytest.raises(P.PvwError, match="either a seed"):
        P.encrypt_party_shares([0] * p.n, 0, gpk, bytes(32), randomness=st)
    shares = [[0] * p.n for _ in range(p.n)]
    with pytest.raises(P.PvwError, match="either a seed"):
        P.encrypt_all_party_shares(shares, gpk, bytes(32), randomness=st)
    with pytest.raises(P.PvwError, match="needs a 32-byte seed or a DeviceRandomness"):
        P.encrypt_all_party_shares(shares, gpk)
    with pytest.raises(P.PvwError, match="has been freed"):
        st.counter()
    st.free()                                                # freeing twice / a never-created handle is a no-op
    assert {"DeviceRandomness"} <= set(P.__all__)


def test_cpp_mirror_compiles_against_the_header():
    exe = os.path.join(ROOT, "build", "device_randomness_cpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "device_randomness.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "pvw_rs_amd"), "-lpvw_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pvw_rs_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "call_seed ok" in out.stdout


def test_rust_mirror_declares_the_entry_points():
    sys_rs = open(os.path.join(ROOT, "rust", "pvw-hip-sys", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS[:-1]:
        assert re.search(r"pub fn " + name + r"\(", sys_rs), name
    crypto = open(os.path.join(ROOT, "rust", "pvw", "src", "crypto.rs")).read()
    assert "pub struct DeviceRandomness" in crypto and "Arc<PvwParameters>" in crypto

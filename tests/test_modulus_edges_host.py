"""CPU checks at the modulus widths the kernels branch on (tests/_util.py MOD_CLASSES, EDGE_CHAINS): the shared arithmetic
of pvw_arith.h against 128-bit remainders, the digit step of the GEMM operands for every q the validator accepts up to 2^16,
the C oracle (what the GPU tests trust) against its plain-remainder build and the big-integer model, and the decode the
device runs, restated on the host, against the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pvw_model as M
import pvw_oracle as O
import pvw_rs_amd as P
from pvw_rs_amd import _ffi
import test_oracle_c as OC
from _util import EDGE_CHAINS, EDGE_MODULI, MIXED_CHAINS, PURE_CHAINS, chain_max_l, decode_cases, primes_1mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "arith_edges.cpp")
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")

# every q in [17, 65537] that validate_params accepts for some l (prime, 1 mod 16): the digit step's small range
SMALL_VALID = [q for q in range(17, 65538) if (q - 1) % 16 == 0 and M.is_prime(q)]


def _run_arith(moduli, *defines):
    exe = os.path.join(ROOT, "build", "arith_edges" + "".join("_" + d.lower() for d in defines))
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC]
                          + ["-D" + d for d in defines] + [SRC, "-o", exe])
    return subprocess.run([exe], input=" ".join(str(q) for q in moduli), capture_output=True, text=True, timeout=600)


def test_arith_header_matches_128_bit_remainders_at_every_width():
    # reduce128 / mulmod / mulmod_shoup / signed_residue / the lazy accumulator up to 2^32 terms / the l-point NTT /
    # the digit step, for every class modulus, the bench chain's moduli and every small q the validator accepts
    moduli = EDGE_MODULI + M.bench_moduli(3) + primes_1mod(128, 2, top=1 << 62) + SMALL_VALID
    out = _run_arith(moduli)
    assert out.returncode == 0 and f"ARITH_EDGES_OK {len(moduli)}" in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]


def test_digit_step_through_the_old_constants_fails_exactly_below_256():
    # The constant pair the digit kernels used before mul256_consts (w = 256, wp = floor(2^128 / q) >> 56) needs w < q:
    # this checker, pointed at that expression, must flag every q < 256 and nothing else (so the test above would
    # have caught the overflow)
    moduli = [q for q in SMALL_VALID if q < 2000] + EDGE_MODULI
    out = _run_arith(moduli, "PVW_PARENT_DIGIT_STEP")
    assert out.returncode == 1
    fails = [ln for ln in out.stdout.splitlines() if ln.startswith("FAIL")]
    assert {ln.split()[1] for ln in fails} == {"digit_step"}, fails
    assert {int(re.search(r"q=(\d+)", ln).group(1)) for ln in fails} == {q for q in moduli if q < 256}


def test_both_digit_kernels_take_their_constants_from_mul256_consts():
    # The kernels' results cannot show which constants the 7-byte digit kernel uses: with the old pair (w = 256) every one
    # of its seven values stays congruent to y 256^a and below 2^56 for q < 256, so its GEMM was exact anyway; only the
    # eighth value of the 8-byte kernel reaches 2^64 (q = 241) and breaks the balanced digits.  Both kernels keep every
    # value reduced below q through the one helper the arithmetic test above checks: the source must say so.
    src = open(os.path.join(CSRC, "pvw_gemm.hip")).read()
    for kernel in ("vec_digits_kernel(", "vec_digits7_kernel("):
        body = src[src.index(kernel):]
        body = body[:body.index("\n}\n")]
        assert "mul256_consts(m, w256, w256p);" in body, kernel
        assert re.search(r"mulmod_shoup\([^;]*, w256, w256p, m\.q\)", body), kernel
    assert not re.search(r"mulmod_shoup\([^;]*,\s*256\s*,", src)
    assert "ratio_hi << 8" not in src


def _geometry(moduli, l):
    return (3, 4, l) if max(moduli) < 1 << 16 else (5, 6, l)


@pytest.mark.parametrize("name", sorted(EDGE_CHAINS))
def test_oracle_barrett_build_agrees_with_plain_build(name):
    # the checker's Barrett reduction against its own 128-bit-remainder build (test_oracle_c.py) on every class chain, at
    # l = 8 and the largest l the chain serves
    moduli = EDGE_CHAINS[name]
    for l in sorted({8, chain_max_l(moduli)}):
        n, k, l = _geometry(moduli, l)
        OC.test_barrett_build_agrees_with_plain_remainder_build(n, k, l, moduli)


@pytest.mark.parametrize("name", sorted(EDGE_CHAINS))
def test_oracle_matches_model(name):
    # keygen, encrypt and decrypt_noisy of the C oracle against the big-integer model, and the model's decode of the
    # result back to the scalars (test_oracle_c.py), at l = 8: every chain here decrypts there
    moduli = EDGE_CHAINS[name]
    OC.test_encrypt_keygen_decrypt_match_model(*_geometry(moduli, 8), moduli)


DECODE_CHAINS = ([(8, MIXED_CHAINS[c], "mixed_" + c) for c in sorted(MIXED_CHAINS)]
                 + [(l, PURE_CHAINS[c], "pure_" + c) for c in ("tiny", "above256") for l in (8,)]
                 + [(l, PURE_CHAINS[c], "pure_" + c) for c in ("bottom62", "top62") for l in (8, 16)]
                 + [(64, [257] + primes_1mod(128, 2), "257_l64")])


@pytest.mark.parametrize("l,moduli", [(l, m) for l, m, _ in DECODE_CHAINS], ids=[i for _, _, i in DECODE_CHAINS])
def test_decode_as_the_device_runs_it_matches_model(l, moduli):
    # the fixed-width decode (host big integers, the fixed-width restatement) and the device's short path restated on the
    # host (pvw_selftest_decode_shortcuts: the kernels' own arithmetic and tables) against decode_scalar_pvw_rns of the model
    p = (P.PvwParametersBuilder().set_parties(3).set_dimension(4).set_l(l).set_moduli(moduli)
         .set_secret_variance(0.5).set_error_bounds(100, 200).build())
    m = M.Params(3, 4, l, moduli)
    cases = decode_cases(l, moduli)
    arr = np.ascontiguousarray(np.array([[[c % q for c in z] for q in moduli] for z in cases], dtype=np.uint64))
    want = [M.decode_scalar_pvw(z, m) for z in cases]
    assert P.decode_scalar_pvw_host(p, arr) == want
    assert P.api._selftest_decode_fixed(p, arr) == want
    out = np.zeros(len(cases), dtype=np.uint64)
    took = np.zeros(len(cases), dtype=np.uint8)
    rc = _ffi.lib().pvw_selftest_decode_shortcuts(p._h, arr.ctypes.data_as(C.c_void_p), len(cases), out.ctypes.data_as(C.c_void_p),
                                                  took.ctypes.data_as(C.c_void_p))
    assert rc == 0, _ffi.last_error()
    assert [int(x) for x in out] == want


@pytest.mark.parametrize("q", [17, 97, 241, 257, 337])
def test_validator_accepts_the_small_classes(q):
    # the range is served, not refused: these are valid moduli for l = 8 (and 257 for every l <= 64)
    for l in (8, 16, 32, 64):
        b = P.PvwParametersBuilder().set_parties(3).set_dimension(4).set_l(l).set_moduli([q, M.bench_moduli(1)[0]] if l <= 32 else [q])
        if (q - 1) % (2 * l) == 0:
            assert b.build().delta() == M.Params(3, 4, l, b._moduli).delta
        else:
            with pytest.raises(P.PvwError):
                b.build()

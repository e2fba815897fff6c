"""Shamir shares over a prime field of up to 256 bits on the device (pvw_shamir_shares_wide*, pvw_deal_shares_wide*, DESIGN
8.18), bit for bit: shamir_eval_wide_kernel against pvw_shamir_shares_wide_host (sharded contexts, n not a multiple of 64 or 256,
D beyond one pass of limb vectors, degrees around the staging chunk, drawn and explicit coefficients, unreduced words); the
kernel's Horner step against Python's integers up to x = 2^32 - 1; the fused deal against pvw_encrypt_multi of the host shares'
limb planes (both sides of the dispatch, both representations, 52- and 62-bit limbs, host-buffer and device-pointer forms); the
_rs forms, their counter and stream capture; the loop closed down to the reconstructed sum of the dealers' secrets over the
secp256k1 order; no share or secret left behind; the host-buffer forms staged in several pieces; the C++ mirror.  Every case
runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_wide_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["shares", "step", "deal", "rs", "loop", "hygiene", "pieces"])
def test_shamir_wide_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_worker.py"), case], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_closes_the_loop_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CPP_OK" in out.stdout, out.stdout + out.stderr

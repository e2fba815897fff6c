"""Packed Shamir dealing over a prime field of up to 256 bits on the device (pvw_shamir_shares_packed_wide*,
pvw_deal_shares_packed_wide*), bit for bit against pvw_shamir_shares_packed_wide_host: the packed kernel and its
weights (n not a multiple of 256 and beyond one workgroup, the secret and Horner chunk edges, D beyond one launch, sharded
contexts, drawn and explicit coefficients, unreduced words, four primes); the fused deal against pvw_encrypt_multi of the host
shares' limb planes (both sides of the dispatch, both representations, 52- and 62-bit limbs, host-buffer and device-pointer
forms, pack = 1 against pvw_deal_shares_wide*); the _rs forms, their counter and stream capture; the loop closed down to the
corrected sums of the dealers' secrets over the secp256k1 order; no share or secret left behind; the host-buffer forms staged in
several pieces and called from several threads; the C++ mirror.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_packed_wide_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["shares", "deal", "rs", "loop", "hygiene", "pieces", "concurrent"])
def test_shamir_packed_wide_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_packed_wide_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_WIDE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_closes_the_loop_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_WIDE_CPP_OK" in out.stdout, out.stdout + out.stderr

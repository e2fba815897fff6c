"""Corrected Shamir reconstruction over a prime field of up to 256 bits on the device (pvw_shamir_reconstruct_wide_corrected*,
DESIGN 8.20), bit for bit against pvw_shamir_reconstruct_wide_corrected_host on out, nerr, col_err and err_mask: small shapes at
every edge of the frame (t + 1 in {1, 2, 4, 5, 33} x r in {0, 1, 2, 3, 8, 9, 126 .. 130}, both layouts, unreduced words, NULL
outputs, four primes, the checked call beside it on a bad share in column 0); the dynamic-LDS opt-in path at count 2052, t 1
against planted truth; the host-buffer form through both copy paths, pieces and passes, and what it leaves behind; stream
capture and replay; the chain deal -> decrypt_all -> fold -> corrected reconstruction in place over the secp256k1 order with
party 0 tampered; the C++ mirror.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_wide_corrected_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small1", "small2", "small4", "small5", "small33", "lds", "pieces", "capture", "loop"])
def test_shamir_wide_corrected_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_corrected_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CORRECTED_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_corrects_a_sharing_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CORRECTED_CPP_OK" in out.stdout, out.stdout + out.stderr

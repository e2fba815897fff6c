"""Shamir reconstruction with erasures over a prime field of up to 256 bits on the device (pvw_shamir_reconstruct_wide_erasures*,
pvw_shamir_wide_erasure_mask_device), bit for bit against pvw_shamir_reconstruct_wide_erasures_host on out, nerr,
col_err and err_mask: small shapes at every edge of the frame (t + 1 in {1, 2, 4, 5, 33} x r in {0, 1, 2, 3, 8, 9, 63, 64, 65,
126 .. 130}, S in 1 .. 9, both layouts, unreduced words, NULL outputs, four primes, every class of erasure and error counts and
random masks, junk at the erased positions); a NULL mask against the wide corrected device call; far rows at p = 65537; the mask
kernel; the dynamic-LDS opt-in path at both of its edges against planted truth; the host-buffer form through both copy paths,
pieces and passes, and what it leaves behind; stream capture with another mask per replay and its refusal; two threads on one
context; the chain deal -> checked decrypt-all -> mask -> fold -> reconstruction in place over the secp256k1 order; the C++
mirror.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_wide_erasures_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small1", "small2", "small4", "small5", "small33", "null", "far", "mask", "ldslo", "ldshi", "pieces",
                                  "capture", "concurrent", "loop"])
def test_shamir_wide_erasures_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_erasures_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_ERASURES_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_reconstructs_with_erasures_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_ERASURES_CPP_OK" in out.stdout, out.stdout + out.stderr

"""Reconstruction with erasures on the device (pvw_shamir_*_erasures*, pvw_shamir_erasure_mask_device), bit for bit
on values, out, nerr, col_err and err_mask against the host forms: the grid t + 1 in {1, 2, 5, 64, 65} x r in {0, 1, 2, 3, 63, 64,
65, 126 .. 131} (one case per t + 1), S rotating through {1, 3, 4, 5, 130} and T through {1, 2, 63, 64, 65, 130}, with the erasure
patterns, error plans and target mixes of the worker, at three primes of which 257 is one; arbitrary words at p = 257, where far
rows decode to polynomials nobody dealt; erased == NULL against the calls extended; the mask builder; the
host-buffer forms, their copy paths, staged pieces, passes, target groups and hygiene; stream capture; a full-size sharing against
planted truth; the protocol loop closed on the device; concurrent calls on one context; the C++ mirror.  Every case runs in a
process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_erasures_host as H

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["grid1", "grid2", "grid5", "grid64", "grid65", "far", "compat", "mask", "buffers", "pieces", "capture", "full", "loop", "concurrent"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_reconstruction_with_erasures_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_erasures_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SHAMIR_ERASURES_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_decodes_with_erasures_on_the_device_as_on_the_host():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ERASURES_CPP_OK" in out.stdout, out.stdout + out.stderr

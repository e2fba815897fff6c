"""Corrected Shamir reconstruction on the device (pvw_shamir_reconstruct_corrected*), bit for bit on out, nerr,
col_err and err_mask against pvw_shamir_reconstruct_corrected_host: the grid t + 1 in {1, 2, 4, 5, 64, 65} x r in {0, 1, 2, 3,
126 .. 131} (one case per t + 1) with no error, one, E, E + 1, errors inside columns 0..t, disjoint error sets and a whole bad
column; the checked call beside the corrected one; the host-buffer form, its copy paths, pieces and hygiene; stream capture; a
full-size sharing against planted truth; the protocol loop closed with tampered parties; the C++ mirror.  Every case runs in a
process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_correct_host as H

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["grid1", "grid2", "grid4", "grid5", "grid64", "grid65", "versus", "buffers", "pieces", "capture", "full", "loop"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_corrected_reconstruction_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_correct_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SHAMIR_CORRECT_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_corrects_on_the_device_as_on_the_host():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CORRECT_CPP_OK" in out.stdout, out.stdout + out.stderr

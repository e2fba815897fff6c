"""Checked Shamir reconstruction on the device (pvw_shamir_reconstruct_checked*), bit for bit on out, bad and
col_bad: shamir_weights_kernel and shamir_interp_kernel against pvw_shamir_reconstruct_checked_host at every edge of the frame
(terms per wave uneven, one chunk and several, a ragged last block of targets, a ragged secret group), both layouts, unreduced
words, explicit corruptions, three primes and a far-apart index set; the host-buffer form, its staged pieces and its hygiene;
stream capture; a full-size sharing made by pvw_shamir_shares_device; more secrets than one launch holds; the protocol loop
closed with every party checked; the C++ mirror.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_check_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["grid", "far", "buffers", "pieces", "capture", "full", "launches", "loop"])
def test_checked_reconstruction_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_check_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SHAMIR_CHECK_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_reports_from_the_device_and_closes_the_loop():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RECONSTRUCT_CPP_OK" in out.stdout, out.stdout + out.stderr

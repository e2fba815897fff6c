"""Shamir shares on the device (pvw_shamir_shares*, pvw_deal_shares*), bit for bit: shamir_eval_kernel against
pvw_shamir_shares_host on the grid of tests/test_shamir_host.py (sharded contexts, n not a multiple of 64, D beyond one pass,
drawn and explicit coefficients); the fused deal against pvw_encrypt_multi of the host shares (both sides of the dealer-count
dispatch, both representations, the 17-limb 61-bit chain and the 4 x 56-bit set, host-buffer and device-pointer forms); the
_rs forms, their counter and stream capture; the loop closed down to the reconstructed sum of the valid dealers' secrets; no
share or secret left behind; config 3 at full size; the C++ mirror.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["shares", "deal", "rs", "loop", "hygiene", "full"])
def test_shamir_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_worker.py"), case], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "SHAMIR_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_closes_the_loop_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_CPP_OK" in out.stdout, out.stdout + out.stderr

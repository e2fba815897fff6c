"""Packed Shamir sharing on the device (pvw_shamir_shares_packed*, pvw_deal_shares_packed*), bit for bit:
shamir_eval_kernel<true> and the device-made weights against pvw_shamir_shares_packed_host at the shapes where the kernel can
go wrong (fewer terms than waves, the secret/random boundary on a wave edge, inside a wave's range and on a chunk edge, several
chunks, D beyond one launch, sharded contexts whose first party is no multiple of 64; drawn and explicit coefficients); the fused
deal against pvw_encrypt_multi of the host shares; the _rs forms, their counter and stream capture; the loop closed down to the
corrected sums of the valid dealers' secrets; nothing secret left behind; staged pieces; concurrent calls; the C++ mirror.
Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_packed_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["shares", "deal", "rs", "loop", "hygiene", "staged", "concurrent"])
def test_packed_shamir_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_packed_worker.py"), case], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_closes_the_loop_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_PACKED_CPP_OK" in out.stdout, out.stdout + out.stderr

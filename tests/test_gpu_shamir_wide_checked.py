"""The receiving end over a prime field of up to 256 bits on the device (pvw_shamir_wide_from_limbs_device,
pvw_shamir_reconstruct_wide_checked*), bit for bit: the kernels' general product against Python's integers; the
fold of limbs against pvw_shamir_wide_from_limbs_host (both stride pairs, words up to 2^64 - 1); the weights and the product
kernel against pvw_shamir_reconstruct_wide_checked_host at the frame's edges (one target, both sides of the 64-target block, of
the four-wave split, of the term chunk and of the secret group; both layouts; planted deviations; unreduced words; NULL counters;
the host-buffer and the device-pointer form); stream capture and replay; the chain deal -> decrypt_all -> fold -> checked
reconstruction in place over the secp256k1 order; staging in several pieces; no share or secret left behind; the C++ mirror.
Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_wide_checked_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mul", "fold", "checked", "capture", "loop", "pieces", "hygiene"])
def test_shamir_wide_checked_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_checked_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CHECKED_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_checks_a_sharing_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_CHECKED_CPP_OK" in out.stdout, out.stdout + out.stderr

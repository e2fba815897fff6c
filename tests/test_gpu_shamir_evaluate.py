"""Share repair on the device (pvw_shamir_evaluate_corrected*), bit for bit on values, out, nerr, col_err and
err_mask against pvw_shamir_evaluate_corrected_host: the grid t + 1 in {1, 2, 5, 64, 65} x r in {0, 1, 2, 3, 126 .. 131} and
t + 1 = 128 x r in {127 .. 130} (one case per t + 1), T rotating through {1, 2, 63, 64, 65, 130} and S through {1, 3, 4, 5, 130},
with the target mixes and error plans of the worker; the host-buffer form, its copy paths, staged pieces, passes, target groups
and hygiene; stream capture; a full-size sharing against planted truth; the protocol loop closed; concurrent calls of
pvw_shamir_reconstruct_corrected and pvw_shamir_evaluate_corrected on one context; the C++ mirror.  Every case runs in a process
of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_evaluate_host as H

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["grid1", "grid2", "grid5", "grid64", "grid65", "grid128", "buffers", "pieces", "capture", "full", "loop", "concurrent"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_share_repair_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_evaluate_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SHAMIR_EVALUATE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_repairs_shares_on_the_device_as_on_the_host():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "EVALUATE_CPP_OK" in out.stdout, out.stdout + out.stderr

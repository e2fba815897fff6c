"""Share repair over a prime field of up to 256 bits on the device (pvw_shamir_evaluate_wide_corrected*,
pvw_shamir_evaluate_wide_erasures*), bit for bit against the _host forms on values, out, nerr, col_err and err_mask:
small shapes at every edge of the frame (t + 1 in {1, 2, 5, 33} x r in {0, 1, 2, 3, 8, 9, 63, 64, 65}, T through {1, 2, 31, 32, 33,
63, 64, 65, 130}, S through {1, 3, 4, 5, 9}, both layouts, unreduced words, NULL optional outputs, four primes, with and without
masks, every class of erasure and error counts, targets on right / wrong / erased columns, off the columns and duplicated, junk at
the erased positions); a NULL mask against the maskless device call and the reports against the decode-only device calls; far
rows at p = 65537 and 257; target groups, secret passes, both copy paths and pieces of the host-buffer form, and what they leave
behind; stream capture and its refusals; two threads on one context; a mid-size repair against planted truth; the chain deal ->
checked decrypt-all -> mask -> fold -> repair in place over the secp256k1 order; the C++ mirror.  Every case runs in a process of
its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_wide_evaluate_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small1", "small2", "small5", "small33", "null", "far", "groups", "capture", "concurrent", "repair",
                                  "loop"])
def test_shamir_wide_evaluate_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_evaluate_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_EVALUATE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_repairs_shares_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_EVALUATE_CPP_OK" in out.stdout, out.stdout + out.stderr

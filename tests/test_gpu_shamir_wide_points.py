"""Wide share repair at field points on the device (pvw_shamir_evaluate_wide_corrected_at*, pvw_shamir_evaluate_wide_erasures_at*,
pvw_shamir_packed_wide_secrets*), bit for bit against the _host forms: `at` (t + 1 in {1, 2, 5} x r in {0, 1, 2, 3, 8},
T through {1, 2, 63, 64, 65, 130}, S through {1, 4, 5}, the points 0, 1, p - 1, p - 2, 2^64, 2^200, points on right, wrong and erased
columns, duplicates and shuffles, both layouts, unreduced words, NULL optional outputs, with and without masks, the device and
the host-buffer form, the index device call reproduced by points = targets + 1, the point 0 equal to out); far rows at p = 65537
and 257; `packed` (K in {1, 2, 5, 64, 65} x t in {0, 1, 4} x r in {0, 1, 2, 5}, wrong shares, erasures, both, an undecodable row,
a [party][row] buffer in place, equality with the older Python route); point groups, secret passes, both copy paths and staged
pieces; what the calls leave behind; stream capture of the packed call and its refusals; two threads on one context; the chain
deal -> aggregate -> checked decrypt-all -> mask -> fold -> packed secrets in place over the secp256k1 order; the C++ mirror.
Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

import test_shamir_wide_points_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["at1", "at2", "at5", "far", "packed1", "packed2", "packed5", "packed64", "packed65", "groups", "hygiene",
                                  "capture", "concurrent", "loop"])
def test_shamir_wide_points_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_points_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_POINTS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_reads_packed_secrets_on_the_device():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_POINTS_CPP_OK" in out.stdout, out.stdout + out.stderr

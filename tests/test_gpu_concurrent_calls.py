"""The concurrent-call promise of the C ABI (include/pvw_hip.h, Conventions), entry point by entry point: threads
that share ONE context make calls that overlap in time -- the context's first encrypts (device initialisation's tail, the first
workspaces, ensure_packed and ensure_xm entered concurrently), a rotating list of every host-buffer kind (a recycled workspace
goes to a call of another kind and size), the same with every staging call in three pieces or more, device-pointer calls on
streams of their own next to host-buffer calls, the _rs forms on a state per thread, and refused calls next to valid ones -- and
every result equals, bit for bit, what a twin context computed serially and the ground truth there is (dealt plaintexts, the
*_host restatements).  A case fails unless calls from different threads did overlap, and unless pvw_selftest_secret_residue finds
nothing afterwards.  The cases and what each asserts: tests/_concurrent_worker.py.  Every case runs in a process of its own under
a time limit (a guard against hangs, not a performance claim).  Measured on an MI355X: 2.2 to 2.7 s of wall time per case, the
start of the process included; the calls of a case take 0.1 to 0.3 s."""
import os
import subprocess
import sys

import pytest

from pvw_rs_amd import _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_concurrent_worker.py")
CASES = ["cold_encrypt-packed56", "cold_encrypt-packed61", "cold_multi", "mixed-packed56", "mixed-plain", "staged", "streams", "rs", "errors"]


def test_worker_comparison_can_fail():
    """no GPU: the worker's comparison reports two swapped expected entries, a flipped bit, a missing result and a changed type;
    its overlap count ignores calls of one thread; its cases are the ones parametrised below"""
    out = subprocess.run([sys.executable, WORKER, "selfcheck"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CONCURRENT_SELFCHECK_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "cases: " + " ".join(sorted(CASES)) in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_concurrent_calls_on_one_context(case):
    if case == "staged" and not os.path.exists(_ffi.LIB_TUNING_PATH):
        pytest.skip("the tuning build is absent")
    out = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CONCURRENT_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "overlapping call pairs" in out.stdout and "residue 0 non-zero" in out.stdout, out.stdout[-3000:]

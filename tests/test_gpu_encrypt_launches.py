"""The launch sequence of the twelve encrypt entry points (pvw_encrypt*, pvw_encrypt_multi*, pvw_deal_shares*; seeds and _rs,
host buffers and device pointers): per-kernel launch counts from the library's own profiling against a recorded table, on both
sides of the matrix-core threshold, past one prologue window and past one GEMM pass, and the _rs counter advanced by exactly D.
The other GPU tests pin what these calls compute; this one pins what they enqueue.  Runs in a process of its own
(tests/_encrypt_launches_worker.py) under a time limit."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_every_encrypt_entry_point_enqueues_the_recorded_launches():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_encrypt_launches_worker.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "LAUNCHES_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

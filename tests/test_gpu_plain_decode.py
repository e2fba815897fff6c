"""The plain decode on the device (pvw_decode_plain*, pvw_decrypt_*_plain*), bit for bit against
pvw_decode_plain_host and the per-dealer host sums: both decode forms on the CPU test's inputs (the fixed-width form and
every-lift-in-full through the tuning build); the aggregate of 64 dealers' field-sized shares through every sum entry point,
both sides of the 22-party dispatch, masks, the resident key; the per-dealer paths with a tampered c2, a wrong key and a
negative share; stream capture with and without pvw_prepare; a sharded context; no key material left behind.  Each case runs
in a child process."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["decode", "aggregate", "perdealer", "capture", "shard"])
def test_plain_decode_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_plain_decode_worker.py"), case], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "PLAIN_DECODE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

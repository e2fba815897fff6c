"""The wide handover on the device, bit for bit against the _host forms: the signed-digit kernel on the edge set at
counts on either side of a wave and a workgroup; the weights kernels (D across the 32-column batch and the 64-lane wave, masks,
T on either side of a wave, targets on valid and masked holders, four primes, both limb widths, four digit widths, a marked
output buffer); the fold over a report read in place; pvw_decrypt_all_handover_wide* over the secp256k1 order on both sides of the
22-party dispatch against the Python truth, against the composition of the three pieces and down to the reconstructed old
secrets, for a plain and a packed old sharing; no share left behind; the host-buffer form staged in several pieces; stream
capture; two threads.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["digits", "weights", "fold", "handover", "hygiene", "pieces", "capture", "threads"])
def test_shamir_wide_handover_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_handover_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_WIDE_HANDOVER_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

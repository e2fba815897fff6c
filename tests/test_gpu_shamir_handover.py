"""The one-word handover with weights from a device-side mask on the device, bit for bit against the _host forms:
the weights kernels (D on either side of the 8-column Cauchy batch, the 64-lane wave and the 256-point upload; no mask, one
holder masked, one holder valid, all masked, only holders beyond lane 63; T in {1, 3, 65}; targets on valid and on masked
holders; three primes; a marked output buffer); the mask kernel on both layouts; pvw_decrypt_all_handover* on both sides of the
22-party dispatch against the composition of the pieces and the Python truth, down to the reconstructed old secrets, for a plain
and a packed old sharing; the mask changed in device memory between two calls and between two replays of one captured call;
corrected reconstruction -> mask -> handover with no host read; no key left behind; staging and target groups in pieces; two
threads.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["weights", "mask", "handover", "remask", "capture", "chain", "hygiene", "pieces", "threads"])
def test_shamir_handover_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_handover_worker.py"), case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SHAMIR_HANDOVER_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

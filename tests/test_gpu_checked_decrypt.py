"""Checked decryption on the device (pvw_decrypt_*_checked, pvw_decode_checked*): values equal the unchecked
calls, noise / status equal the host implementation that computes every residual by its definition -- honest shares from
single- and multi-dealer encrypts, tampered c2, a wrong key or party index, uniform residues, a lossy plaintext, both sides
of the 22-party dispatch, the resident key, both decode forms of the tuning build -- and no key material left behind."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_checked_decryption_on_the_device():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_checked_decrypt_worker.py")], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and "CHECKED_DECRYPT_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

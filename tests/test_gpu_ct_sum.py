"""Sums of dealers' ciphertexts on the device (pvw_ct_sum*, pvw_decrypt_sum_*, pvw_decrypt_all_sum_*), bit for bit:
the kernels (unsplit and split forms, masks, counts, row ranges, a caller's stream, production geometries) against
pvw_ct_sum_host; the aggregate decrypts against the per-dealer decrypts and against pvw_decode_checked_host on the noisy
polynomial of the host-summed ciphertext (both sides of the 22-party dispatch, the resident key, lossy sums, saturated noise);
no key material left behind; stream capture with and without pvw_prepare; a sharded context."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sums", "big", "decrypt", "capture", "shard"])
def test_ciphertext_sums_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_ct_sum_worker.py"), case], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "CT_SUM_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

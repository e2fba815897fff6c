"""Many weighted sums of the same dealers' ciphertexts on the device (pvw_ct_lincomb_many*, pvw_decrypt_all_lincomb_many_plain*,
DESIGN 8.15), bit for bit: the row-tile kernel (every tile size, unsplit and split forms, masks, weights of every kind, rows
nobody takes part in, counts, row ranges, a caller's stream, one shape that is unsplit by itself) and the host-buffer form against
pvw_ct_lincomb_many_host, R = 1 against pvw_ct_lincomb_device; several staged pieces against one; the packed handover (re-deal
the old packed shares, combine with the Lagrange weights at the points -m, one decrypt of all combinations) against
pvw_shamir_shares_host on both sides of the 22-party dispatch, column by column against the single-combination call; no key
material left behind; stream capture; two threads on one context."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["combos", "pieces", "handover", "hygiene", "capture", "threads"])
def test_many_ciphertext_combinations_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_ct_lincomb_many_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CT_LINCOMB_MANY_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

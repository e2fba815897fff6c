"""Weighted sums of dealers' ciphertexts on the device (pvw_ct_lincomb*, pvw_decrypt_lincomb_*, pvw_decrypt_all_lincomb_*,
DESIGN 8.12), bit for bit: the kernel (unsplit and split forms, masks, weights of every kind, counts, row ranges, a caller's
stream, one production shape) and the host-buffer form against pvw_ct_lincomb_host; several staged pieces against one; the
committee handover (deal the old shares again, combine with the Lagrange weights of the valid old holders, one decrypt a
party) against pvw_shamir_shares_host on both sides of the 22-party dispatch, with the one-party forms, the resident key, wide
words and the checked word; no key material left behind; stream capture with and without pvw_prepare, replayed with changed
weights and mask; two threads on one context."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["combos", "pieces", "big", "decrypt", "capture", "threads"])
def test_ciphertext_combinations_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_ct_lincomb_worker.py"), case], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "CT_LINCOMB_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

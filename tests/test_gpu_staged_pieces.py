"""The multi-piece staging of every host-buffer call in pvw_capi.hip, at small shapes: the tuning build with a small staging
budget (PVW_STAGE_BYTES) takes ct_sum_staged, decrypt_batch_staged, both sides of pvw_decrypt_all, the passes of
pvw_encrypt_multi / pvw_deal_shares and pvw_shamir_shares through two or more pieces, and every result is compared bit for bit
with an independent host reference and with the same call in one piece.  real_bound runs the shipped library at a size that
crosses the 1 GiB constant itself.  The cases and what each asserts: tests/_staged_pieces_worker.py."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sum", "sum_decrypt", "batch", "all", "encrypt", "shamir", "real_bound"])
def test_host_buffer_calls_in_several_staged_pieces(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_staged_pieces_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "STAGED_PIECES_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pieces" in out.stdout or "passes" in out.stdout or "chunks" in out.stdout      # every case prints the pieces its calls took

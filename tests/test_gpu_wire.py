"""Wire format v1 on the device: pvw_wire_pack / unpack kernels bit-identical to the host codec over every chain,
ring degree and count the CPU tests use and on 272 MiB of words; output into pvw_host_alloc memory; the exact count of
rejected residues; public keys and CRS rows through pvw_get_*_wire / pvw_load_*_wire, encrypting as pvw_load_pk does on both
encrypt paths, atomic on rejection; ciphertexts and keys moved to a second context decrypting to the dealt values; a sharded
context's blobs; the C++ mirror."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_wire_format_on_the_device():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_wire_worker.py")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "WIRE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

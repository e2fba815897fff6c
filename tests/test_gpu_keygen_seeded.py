"""Key generation from a seed on the device (pvw_keygen_seeded, pvw_sample_secret_keys_device, pvw_sk_load_seeded),
everything bit for bit: B-hat against the C oracle on the oracle's own draw of the keys and against pvw_sample_secret_keys +
pvw_keygen, one shape per branch (VALU, k = 1, transposed GEMM, the drawn shat_mftile with ragged rows and k, l = 32, the l = 64
prologue branch, two chunks), each with distinct and with equal seeds; sub-ranges of a pre-filled key by global index; variances
1, 3 and 10; sharded contexts; the tuning library's other two forms; drawn keys in device memory feeding pvw_decrypt_all_device;
the resident key against pvw_sk_load; key hygiene after each call; the protocol loop.  Every case runs in a process of its own
under a time limit."""
import os
import subprocess
import sys

import pytest

import test_keygen_seeded_host as H

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["paths-valu", "paths-k1", "paths-transposed", "paths-swapped", "paths-l32", "paths-l64", "paths-chunks",
         "range", "variance", "sharded", "tuning", "sk_device", "resident", "hygiene", "loop"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_key_generation_from_a_seed_on_the_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_keygen_seeded_worker.py"), case], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "KEYGEN_SEEDED_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_mirror_generates_the_two_step_key_from_a_seed():
    H._build_cpp()
    out = subprocess.run([H.EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "KEYGEN_SEEDED_CPP_OK" in out.stdout, out.stdout + out.stderr

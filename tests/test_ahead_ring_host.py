"""The bookkeeping of the encrypt's ahead ring (pvw_rs_amd/csrc/pvw_ahead_ring.h: which set a call takes, when the guard of a
bank is recorded and waited for) against a model of the two streams: tests/cpp/ahead_ring.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ahead_ring.cpp")
CSRC = os.path.join(ROOT, "pvw_rs_amd", "csrc")


def test_ahead_ring_bookkeeping_under_sanitizers():
    exe = os.path.join(ROOT, "build", "ahead_ring")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # the sanitizer runtimes are linked statically, so the program needs no LD_PRELOAD and no particular library order
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "AHEAD_RING_OK" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]

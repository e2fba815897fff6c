"""The ahead path of the seed-mode encrypt: while the previous call's MAC is outstanding on the caller's stream the prologue runs
on a side stream into a ring of (r-hat, e_small) sets and the MAC is enqueued, once the calling thread has seen the prologue
finish, with nothing in front of it (encrypt_enqueue).  Bit-exactness against the same calls made alone on an idle
stream and against the C oracle, across the ring's wrap, with the caller's own stream order, in mixed sequences and from two
threads; and which calls take the path.  Three tiny geometries, one for each MAC kernel with compact addends: A n = 48, k = 256,
l = 8, three 61-bit limbs (packed61); B n = 20, k = 64, l = 16, two 56-bit limbs (packedw); C n = 12, k = 24, l = 8, two limbs
(unpacked).  Each case runs in a process of its own (tests/_encrypt_ahead_worker.py) under a time limit."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(*case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_encrypt_ahead_worker.py"), *case], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "AHEAD_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", ["A", "B", "C"])
def test_twelve_calls_on_a_busy_stream_equal_the_calls_made_alone(geometry):
    _run("exact", geometry)


@pytest.mark.gpu
def test_caller_data_stays_ordered_by_the_callers_stream():
    _run("ordered")


@pytest.mark.gpu
def test_which_calls_take_the_ahead_path():
    _run("paths")


@pytest.mark.gpu
def test_mixed_sequence_of_seed_rs_and_explicit_calls():
    _run("mixed")


@pytest.mark.gpu
def test_two_threads_on_two_busy_streams():
    _run("concurrent")

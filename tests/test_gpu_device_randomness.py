"""Encrypt from a device randomness state (pvw_rnd_state): eager calls, graph replays and multi-dealer calls draw
call_seed(S, c + i) when their kernels run and advance the counter on the device, so replays get fresh randomness.  Each
case runs in a fresh process (tests/_device_rnd_worker.py: torch first, then the library, on torch streams)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def _run(case, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_device_rnd_worker.py"), case], capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0 and "RND_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_eager_single_dealer_matches_seed_mode_and_advances():
    _run("eager_single")


def test_graph_replays_draw_fresh_randomness():
    _run("graph_single")


def test_multi_dealer_both_paths_and_captured_replays():
    _run("multi", timeout=900)


def test_multi_dealer_capture_without_prepare_is_refused_cleanly():
    _run("capture_unprepared")


def test_free_clears_the_device_seed():
    _run("free_clears")

"""The 256-bit Shamir family on the device at every prime width its arithmetic branches on (WIDE_PRIME_CLASSES of
tests/_util.py): the step and product selftests, the share kernels (plain and packed), the fused deal, the
limb fold, checked, corrected and erasure reconstruction, share repair, and the handover's digits, weights and fold.  At every
one of the 24 primes the device equals the _host form bit for bit, and both equal the big-integer expectation of
tests/test_shamir_wide_prime_edges_host.py.  Every case runs in a process of its own under a time limit and reports how many
(family, prime) pairs it ran and which of them ended in an asserted refusal."""
import os
import re
import subprocess
import sys

import pytest

from _util import WIDE_EDGE_PRIMES, WIDE_PRIME_CLASSES

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = ["step", "mul", "shares", "packed", "deal", "fold", "checked", "corrected", "erasures", "evaluate", "digits", "weights", "from_digits"]
# the (family, prime) pairs whose every shape the contract refuses, where the worker asserts the refusal instead: none.  The
# shapes follow the field down (p = 3: two parties, two shares of degree 0, a pack of one), so every pair runs.
REFUSALS = []


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_wide_family_at_every_prime_width_on_the_device(family):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_shamir_wide_prime_edges_worker.py"), family], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    done = re.search(r"^SHAMIR_WIDE_PRIME_EDGES_OK (\w+) pairs=(\d+) refusals=(.*)$", out.stdout, re.M)
    assert done and done.group(1) == family, out.stdout[-3000:] + out.stderr[-3000:]
    # the deal runs one prime of every class, every other family all the primes; none is left out or refused
    assert int(done.group(2)) == (len(WIDE_PRIME_CLASSES) if family == "deal" else len(WIDE_EDGE_PRIMES))
    assert done.group(3) == repr(sorted(pair for pair in REFUSALS if pair[0] == family))

"""CPU checks of the plain decode: the decode finished in the caller's modulus, or handed back as the wide
integer.  The host big-integer implementation (pvw_decode_plain_host) and the fixed-width device algorithm run on the host
(pvw_selftest_decode_plain) against the contract restated in tests/_plain_cases.py from the model's integers, on every input
at eight parameter sets and seven moduli; with no option set both equal the checked decode bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pvw_model as M
import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
import _plain_cases as PC
import test_checked_decode_host as TC


def _setup(name):
    moduli, l = PC.SETS[name]
    return TC._params(moduli, l), M.Params(3, 4, l, moduli), moduli


def _compare(tag, r, want, ww):
    w_out, w_noise, w_status, w_wide = want
    for what, got, exp in (("out", r.residues, w_out), ("noise", r.noise, w_noise), ("status", r.status, w_status)):
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (tag, what, [(int(i), int(got[i]), int(exp[i])) for i in bad[:5]])
    if ww:
        wide = np.array([[(abs(int(v)) >> (64 * w)) & PC.U64 for w in range(ww)] for v in r.values], dtype=np.uint64)
        assert np.array_equal(wide, w_wide), (tag, "wide")


@pytest.mark.parametrize("name", sorted(PC.SETS))
def test_plain_decode_host_and_device_algorithm_match_the_contract(name):
    p, m, moduli = _setup(name)
    cases = PC.all_cases(m)
    noisy = PC.rns(cases, moduli)
    big = PC.unreduce(noisy, moduli)
    assert (big != noisy).any()
    seen = 0
    for modulus, ww in PC.option_grid(m):
        want = PC.contract_arrays(cases, m, modulus, ww)
        for tag, fn in (("host", P.decode_scalar_pvw_plain_host), ("selftest", api._selftest_decode_plain)):
            _compare((tag, modulus, ww), fn(p, noisy, modulus, ww), want, ww)
            _compare((tag, modulus, ww, "unreduced words"), fn(p, big, modulus, ww), want, ww)
        seen |= int(np.bitwise_or.reduce(want[2]))
    # the inputs reach every status bit
    assert seen == PC.DEC_LOSSY | PC.DEC_NEGATIVE | PC.DEC_WIDE_TRUNCATED


@pytest.mark.parametrize("name", sorted(PC.SETS))
def test_chosen_plaintexts_inside_the_radius_come_back_exactly(name):
    """the claim the feature rests on: for |P| < Q/2 and noise inside the radius the decode's P is the P that was put in"""
    p, m, moduli = _setup(name)
    pairs, cases = PC.chosen(m), PC.chosen_cases(m)
    W = PC.q_words(m)
    q0 = int(moduli[0])
    r = P.decode_scalar_pvw_plain_host(p, PC.rns(cases, moduli), q0, None)
    s = api._selftest_decode_plain(p, PC.rns(cases, moduli), q0, W)
    for i, (pl, e) in enumerate(pairs):
        want = M.center(pl % m.Q, m.Q)
        assert int(r.values[i]) == want == int(s.values[i]), (i, pl)
        assert int(r.residues[i]) == want % q0 == int(s.residues[i])
        assert int(r.noise[i]) == min(max(abs(x) for x in e), PC.U64)
        assert bool(r.negative[i]) == (want < 0) and not r.truncated[i]


@pytest.mark.parametrize("name", sorted(PC.SETS))
def test_without_options_it_is_the_checked_decode_bit_for_bit(name):
    p, m, moduli = _setup(name)
    noisy = PC.rns(PC.all_cases(m), moduli)
    for plain_fn, checked_fn in ((P.decode_scalar_pvw_plain_host, P.decode_scalar_pvw_checked_host),
                                 (api._selftest_decode_plain, api._selftest_decode_checked)):
        a, b = plain_fn(p, noisy, 0, 0), checked_fn(p, noisy)
        assert np.array_equal(a.values, b.values) and np.array_equal(a.noise, b.noise) and np.array_equal(a.status, b.status)


def test_argument_errors_come_before_any_work():
    p, m, moduli = _setup("example128_l8")
    lib = _ffi.lib()
    W = PC.q_words(m)
    noisy = PC.rns(PC.chosen_cases(m)[:2], moduli)
    out, noise, status = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    wide = np.zeros((2, W + 1), np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for fn in ("pvw_decode_plain_host", "pvw_selftest_decode_plain", "pvw_decode_plain"):
        call = lambda modulus, ww, wd: getattr(lib, fn)(p._h, ptr(noisy), 2, ptr(out), ptr(noise), ptr(status), modulus, ww, wd)
        for modulus, ww, wd in ((1, 0, None), (1 << 62, 0, None), ((1 << 64) - 1, 0, None), (0, W + 1, ptr(wide)), (3, 1, None)):
            assert call(modulus, ww, wd) == 1, (fn, modulus, ww)                # PVW_ERR_INVALID_PARAMETERS
            assert _ffi.last_error()
    assert lib.pvw_decode_plain_host(p._h, ptr(noisy), 2, ptr(out), ptr(noise), ptr(status), (1 << 62) - 1, W, ptr(wide)) == 0
    with pytest.raises(P.PvwError):
        P.decode_scalar_pvw_plain_host(p, noisy, 1)


def test_python_mirror_reports_values_sign_and_validity():
    p, m, moduli = _setup("example128_l8")
    D, Q = m.delta, m.Q
    cases = [[(-(msg * D ** j) + (amp if j == 3 else 0)) % Q for j in range(m.l)]
             for msg, amp in ((7, 10), (7, 11), (-1001, 0), (1 << 64, 0), (-5, 3))]
    r = P.decode_scalar_pvw_plain_host(p, PC.rns(cases, moduli), 1000, None, bound=10)
    assert [int(v) for v in r.values] == [7, 7, -1001, 1 << 64, -5]
    assert list(r.residues) == [7, 7, (-1001) % 1000, (1 << 64) % 1000, 995]
    assert list(r.lossy) == [False, False, True, True, True]
    assert list(r.negative) == [False, False, True, False, True]
    assert list(r.valid) == [True, False, True, True, True]                    # exact whatever lossy says: the noise test only

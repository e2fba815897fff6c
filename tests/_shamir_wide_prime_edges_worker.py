"""The 256-bit Shamir family on the device at every prime width its arithmetic branches on (WIDE_EDGE_PRIMES of tests/_util.py;
DESIGN 8.18 - 8.24).  One case per family; every case walks all the primes (the deal: one prime of every class) and asserts, at
each, that the device equals the _host form bit for bit and that both equal the big-integer expectation built by
tests/test_shamir_wide_prime_edges_host.py.  The shapes are the smallest that run every kernel of the family: the geometry edges
(waves, workgroups, chunks) are the other workers' business, at four primes.  Every shape below is legal at every prime (the
builders cut it down to the field: p = 3 serves two shares of degree 0), so no (family, prime) pair ends in a refusal; the
worker counts the pairs it ran and lists the refusals it asserted, and the test holds the list to its own.  torch is imported
FIRST so both libraries share one HIP runtime.  Spawned case by case by tests/test_gpu_shamir_wide_prime_edges.py; prints
SHAMIR_WIDE_PRIME_EDGES_OK <family> pairs=<n> refusals=<list>."""
import os
import random
import sys

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_model as M  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from _util import WIDE_EDGE_PRIMES, WIDE_PRIME_CLASSES  # noqa: E402
from test_shamir_wide_host import ints, seeds_for  # noqa: E402
from test_shamir_wide_handover_host import digits_ref, weights_ref  # noqa: E402
import test_shamir_wide_prime_edges_host as H  # noqa: E402
from _shamir_wide_worker import deal_device, device_shares, flat, same as same_cts, system, two_step  # noqa: E402
from _shamir_packed_wide_worker import device_shares as device_shares_packed  # noqa: E402
from _shamir_wide_checked_worker import (DEV, _params, buffer_checked, dev, device_checked, host_checked, nptr, same, u64, words)  # noqa: E402
from _shamir_wide_corrected_worker import buffer_corrected, device_corrected, host_corrected  # noqa: E402
from _shamir_wide_erasures_worker import buffer_erasures, device_erasures, host_erasures, pack  # noqa: E402
from _shamir_wide_evaluate_worker import buffer_evaluate, device_evaluate, host_evaluate  # noqa: E402
from _shamir_wide_handover_worker import device_weights  # noqa: E402

# the host-buffer forms run at one prime of every class: the smallest of the tiny ones, and the word-move-only and wrapped ones
ONE_PER_CLASS = (3, 65537, 2**64 - 59, 2**128 - 159, 2**256 - 189)
DEAL_PRIMES = (251, 65537, 2**64 - 59, 2**128 - 159, 2**256 - 189)
LAYOUTS = H.LAYOUTS
REFUSED = []                     # (family, prime) pairs that ended in an asserted refusal


def to_words(values):
    """ints below 2^256 -> uint64 [N][4] (api._wide through bytes: the selftests take thousands of operands a prime)"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def from_words(a):
    raw = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def step():
    """pvw_selftest_shamir_wide_step == (acc x + add) mod p: 0, 1, p - 1 and 60 random operands in every pairing, under the
    multipliers 1, 2, 2^16 and 2^32 - 1"""
    lib = _ffi.lib()
    p = _params(3)
    for pm in WIDE_EDGE_PRIMES:
        rng = random.Random(pm & 0xFFFFFF)
        ops = [0, 1, pm - 1] + [rng.randrange(pm) for _ in range(60)]
        cases = [(a, x, b) for a in ops for b in ops for x in (1, 2, 1 << 16, (1 << 32) - 1)]
        acc, add = to_words([c[0] for c in cases]), to_words([c[2] for c in cases])
        x = np.array([c[1] for c in cases], dtype=np.uint64)
        out = np.zeros((len(cases), 4), dtype=np.uint64)
        api._check(lib.pvw_selftest_shamir_wide_step(p._h, nptr(api._wide_modulus(pm)), nptr(acc), nptr(x), nptr(add), len(cases), nptr(out)), lib)
        assert from_words(out) == [(a * xx + b) % pm for a, xx, b in cases], hex(pm)
    return len(WIDE_EDGE_PRIMES)


def mul():
    """pvw_selftest_shamir_wide_mul == a b mod p on the same operands in every pairing"""
    lib = _ffi.lib()
    p = _params(3)
    for pm in WIDE_EDGE_PRIMES:
        rng = random.Random(pm & 0xFFFFFF)
        ops = [0, 1, pm - 1] + [rng.randrange(pm) for _ in range(60)]
        cases = [(a, b) for a in ops for b in ops]
        a, b = to_words([c[0] for c in cases]), to_words([c[1] for c in cases])
        out = np.zeros((len(cases), 4), dtype=np.uint64)
        api._check(lib.pvw_selftest_shamir_wide_mul(p._h, nptr(api._wide_modulus(pm)), nptr(a), nptr(b), len(cases), nptr(out)), lib)
        assert from_words(out) == [x * y % pm for x, y in cases], hex(pm)
    return len(WIDE_EDGE_PRIMES)


def _dealing(pack):
    """the share kernels at D = 3, n = min(9, p - pack) and the degrees 0, 1 and the largest, explicit and drawn coefficients, the
    words 0, p - 1, p and 2^256 - 1 among the secrets and the coefficients: device pointer == host == integers, and the
    host-buffer form at one prime of every class"""
    s = torch.cuda.Stream(device=DEV)
    for pm in WIDE_EDGE_PRIMES:
        n, K, degrees = H.dealing_shape(pm, pack)
        p = _params(n)
        for t in degrees:
            secrets, coeffs, seeds = H.dealing_case(pm, n, K, t, 3)
            explicit, drawn = H.dealing_expected(pm, n, K, secrets, coeffs, seeds, t)
            for kw, expect in ((dict(coeffs=coeffs), explicit), (dict(seeds=seeds), drawn)):
                if pack == 1:
                    se = [row[0] for row in secrets]
                    want = P.shamir_shares_wide(p, se, t, pm, host=True, **kw)
                    got = device_shares(p, se, t, pm, stream=s, **kw)
                    buffered = P.shamir_shares_wide(p, se, t, pm, **kw) if pm in ONE_PER_CLASS else want
                else:
                    want = P.shamir_shares_packed_wide(p, secrets, K, t, pm, host=True, **kw)
                    got = device_shares_packed(p, secrets, K, t, pm, stream=s, **kw)
                    buffered = P.shamir_shares_packed_wide(p, secrets, K, t, pm, **kw) if pm in ONE_PER_CLASS else want
                assert np.array_equal(got, want) and np.array_equal(buffered, want), (hex(pm), K, t, list(kw))
                assert ints(want) == expect, (hex(pm), K, t, list(kw))
    return len(WIDE_EDGE_PRIMES)


def shares():
    return _dealing(1)


def packed():
    return _dealing(3)


def deal():
    """pvw_deal_shares_wide at one prime of every class, n = min(5, p - 1), k = 32, l = 8: the ciphertexts of the one call equal
    pvw_encrypt_multi of the host shares' limb planes under the same seeds (host-buffer and device-pointer forms), and the host
    shares are the integers'"""
    assert [any(pm in c for pm in DEAL_PRIMES) for c in WIDE_PRIME_CLASSES.values()] == [True] * 5
    s = torch.cuda.Stream(device=DEV)
    k, l, lb, D = 32, 8, 52, 2
    for pm in DEAL_PRIMES:
        n = min(5, pm - 1)
        t = n - 1
        p, gpk, _ = system(M.bench_moduli(3), n, k, l)
        nl = P.shamir_wide_limbs(pm, lb)
        secrets, _, seeds = H.dealing_case(pm, n, 1, t, D)
        secrets, seeds = [row[0] for row in secrets], seeds_for(D * nl, tag=nl)
        want = two_step(p, gpk, secrets, t, pm, seeds, lb, P.REPR_NTT)
        got = flat(P.deal_party_shares_wide(secrets, t, pm, gpk, seeds=seeds, limb_bits=lb, out_repr=P.REPR_NTT))
        assert same_cts(got, want), ("host-buffer", hex(pm))
        g1, g2 = deal_device(p, secrets, t, pm, lb, P.REPR_NTT, s, seeds=seeds)
        for v in range(D * nl):
            assert np.array_equal(g1[v], want[v].c1) and np.array_equal(g2[v], want[v].c2), ("device", hex(pm), v)
        sh = ints(P.shamir_shares_wide(p, secrets, t, pm, seeds=seeds[::nl], host=True))
        assert sh == [H.evaluate(secrets[d], H.restated_coeffs(seeds[d * nl], t, pm), n, pm) for d in range(D)], hex(pm)
    return len(DEAL_PRIMES)


def fold():
    """pvw_shamir_wide_from_limbs_device at count = 70, both layouts, limbs of 16, 52 and 62 bits, words up to 2^64 - 1"""
    p = _params(3)
    s = torch.cuda.Stream(device=DEV)
    for pm in WIDE_EDGE_PRIMES:
        for lb in H.LIMB_WIDTHS:
            nl, planes, expect = H.limb_case(pm, lb, 70)
            want = P.shamir_wide_from_limbs(planes, pm, lb)
            assert want == expect, (hex(pm), lb)
            got = P.shamir_wide_from_limbs_device(p, dev(planes), pm, lb, stream=s)
            s.synchronize()
            assert ints(u64(got)) == want, ("limb_major", hex(pm), lb)
            got = P.shamir_wide_from_limbs_device(p, dev(np.ascontiguousarray(planes.T)), pm, lb, layout="limb_minor", stream=s)
            s.synchronize()
            assert ints(u64(got)) == want, ("limb_minor", hex(pm), lb)
    return len(WIDE_EDGE_PRIMES)


def checked():
    """count = min(12, p - 1), t = 3 (cut down with the field), S = 3, both layouts: clean rows of unreduced words, then deviating
    extra shares"""
    p = _params(3)
    s = torch.cuda.Stream(device=DEV)
    for pm in WIDE_EDGE_PRIMES:
        case = H.Receiving(pm)
        for name, rows, bad, col_bad in case.checked_scenarios():
            w = words([v for row in rows for v in row], (case.S, case.count))
            for layout in LAYOUTS:
                want = host_checked(case.idx, w, case.t, pm, layout)
                assert (ints(want[0]), want[1].tolist(), want[2].tolist()) == (case.secrets, bad, col_bad), (hex(pm), name, layout)
                assert same(device_checked(p, case.idx, w, case.t, pm, layout, s), want), ("device", hex(pm), name, layout)
                if pm in ONE_PER_CLASS:
                    assert same(buffer_checked(p, case.idx, w, case.t, pm, layout), want), ("host-buffer", hex(pm), name, layout)
    return len(WIDE_EDGE_PRIMES)


def report_of(res):
    """(secrets, nerr, col_err, mask bits) of a raw (out, nerr, col_err, err_mask)"""
    return ints(res[0]), res[1].tolist(), res[2].tolist(), H.mask_bits(res[3])


def _decode(masked):
    """the corrected call on the scenarios without a mask, or the erasures call on those with one and two flagged columns"""
    p = _params(3)
    s = torch.cuda.Stream(device=DEV)
    for pm in WIDE_EDGE_PRIMES:
        case = H.Receiving(pm)
        ran = 0
        for name, rows, erased, report, _ in case.scenarios():
            if (erased is not None) != masked:
                continue
            ran += 1
            w = words([v for row in rows for v in row], (case.S, case.count))
            er = pack([[c for c in range(case.count) if row[c]] for row in erased], case.count) if masked else None
            for layout in LAYOUTS:
                if masked:
                    want = host_erasures(case.idx, w, case.t, pm, er, layout)
                    got = device_erasures(p, case.idx, w, case.t, pm, er, layout, s)
                    buffered = buffer_erasures(p, case.idx, w, case.t, pm, er, layout) if pm in ONE_PER_CLASS else want
                else:
                    want = host_corrected(case.idx, w, case.t, pm, layout)
                    got = device_corrected(p, case.idx, w, case.t, pm, layout, s)
                    buffered = buffer_corrected(p, case.idx, w, case.t, pm, layout) if pm in ONE_PER_CLASS else want
                assert report_of(want) == report, (hex(pm), name, layout)
                assert same(got, want) and same(buffered, want), (hex(pm), name, layout)
        assert ran == 2
    return len(WIDE_EDGE_PRIMES)


def corrected():
    return _decode(False)


def erasures():
    return _decode(True)


def evaluate():
    """the evaluate calls on every scenario, with and without a mask, at five targets: the largest legal index, right, wrong and
    erased columns and an index that is no column's"""
    p = _params(3)
    s = torch.cuda.Stream(device=DEV)
    for pm in WIDE_EDGE_PRIMES:
        case = H.Receiving(pm)
        T = len(case.targets)
        for name, rows, erased, report, values in case.scenarios():
            w = words([v for row in rows for v in row], (case.S, case.count))
            er = None if erased is None else pack([[c for c in range(case.count) if row[c]] for row in erased], case.count)
            for layout in LAYOUTS:
                want = host_evaluate(case.idx, w, case.t, pm, er, case.targets, layout)
                flat_values = ints(want[0].reshape(case.S * T, 4))
                assert [flat_values[i * T:(i + 1) * T] for i in range(case.S)] == values, (hex(pm), name, layout)
                assert report_of(want[1:]) == report, (hex(pm), name, layout)
                got = device_evaluate(p, case.idx, w, case.t, pm, er, case.targets, layout, s, maskless=er is None)
                assert same(got, want), ("device", hex(pm), name, layout)
                if pm in ONE_PER_CLASS:
                    assert same(buffer_evaluate(p, case.idx, w, case.t, pm, er, case.targets, layout), want), ("host-buffer", hex(pm), name)
    return len(WIDE_EDGE_PRIMES)


GPU_DIGIT_WIDTHS = (8, 32, 33, 64)


def digits():
    """pvw_shamir_wide_signed_digits_device on N = 65 values"""
    p = _params(3)
    for pm in WIDE_EDGE_PRIMES:
        for b in GPU_DIGIT_WIDTHS:
            vals = H.digit_values(pm, b, 65)
            want = P.shamir_wide_signed_digits(None, vals, pm, b, host=True)
            assert want.tolist() == [digits_ref(x, pm, b) for x in vals], (hex(pm), b)
            assert np.array_equal(P.shamir_wide_signed_digits(p, vals, pm, b), want), (hex(pm), b)
    return len(WIDE_EDGE_PRIMES)


def weights():
    """pvw_shamir_wide_handover_weights_device: D = 5 holders (the field's own number where it has fewer) with the second masked
    out, the targets 0, p - 1 and a holder's point, limbs of 52 and 62 bits"""
    p = _params(3)
    s = torch.cuda.Stream(device=DEV)
    for pm in WIDE_EDGE_PRIMES:
        idx, valid, points = H.weights_case(pm)
        for b in GPU_DIGIT_WIDTHS:
            for lb in (52, 62):
                want = P.shamir_wide_handover_weights(None, idx, pm, valid, points, lb, b, host=True)
                assert want.tolist() == weights_ref(pm, idx, valid, points, lb, b), (hex(pm), b, lb)
                got, intact = device_weights(p, idx, pm, valid, points, lb, b, s)
                assert intact and np.array_equal(got, want), (hex(pm), b, lb)
    return len(WIDE_EDGE_PRIMES)


def from_digits():
    """pvw_shamir_wide_from_digits_device at count = 70"""
    p = _params(3)
    for pm in WIDE_EDGE_PRIMES:
        for b in GPU_DIGIT_WIDTHS:
            wide, status, expect, est = H.fold_case(pm, b, 70)
            want = P.shamir_wide_from_digits(None, wide, status, pm, b, host=True)
            assert want[0] == expect and want[1].tolist() == est, (hex(pm), b)
            got = P.shamir_wide_from_digits(p, wide, status, pm, b)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]), (hex(pm), b)
    return len(WIDE_EDGE_PRIMES)


CASES = {f.__name__: f for f in (step, mul, shares, packed, deal, fold, checked, corrected, erasures, evaluate, digits, weights, from_digits)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    pairs = CASES[sys.argv[1]]()
    print(f"SHAMIR_WIDE_PRIME_EDGES_OK {sys.argv[1]} pairs={pairs} refusals={sorted(REFUSED)}")

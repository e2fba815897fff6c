"""The 256-bit Shamir family at every prime width its arithmetic branches on (WIDE_PRIME_CLASSES in
tests/_util.py), the CPU half: the stand-alone mirrors under the sanitizers, and the host forms of dealing, the limb helpers, the
receiving end and the handover's public arithmetic against Python's own integers.  Every expectation is made here in integers,
on sharings the test deals itself: the dealt secrets, the planted deviations (never more than the unique-decoding radius, so no
decoder is needed), the polynomials at the targets.  The builders below are shared with the device half
(tests/_shamir_wide_prime_edges_worker.py).  No device is used.

Two readings of the shapes, where a field is too small for the usual ones: the points of `count` shares are distinct and
non-zero, so count = min(12, p - 1) and the degree follows (receiving_shape); a target of the evaluate calls is a party index
whose point index + 1 is below p, so the point 0 is the secret the same call reports and the point p - 1 is the target p - 2
(for p above 2^64 the largest target is 2^64 - 1); the handover weights take field elements and get 0 and p - 1 themselves."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import pvw_rs_amd as P
from _util import WIDE_EDGE_PRIMES, WIDE_PRIME_CLASSES, WIDE_SECP_N, wide_branches
from test_shamir_wide_host import COMPOSITE_255, CSRC, ROOT, SECP_N, W256, evaluate, ints, params, restated_coeffs, seeds_for
from test_shamir_packed_wide_host import packed_evaluate
from test_shamir_wide_handover_host import (build_kernel_sequence, compare_kernel_sequence, digits_ref, edge_set, fold_ref, num_digits,
                                            weights_ref)

U64 = (1 << 64) - 1
UNDECODABLE = P.SHAMIR_UNDECODABLE
PID = lambda p: f"{p.bit_length()}bit_{p & 0xFFFF:04x}"
LIMB_WIDTHS = (16, 52, 62)
DIGIT_WIDTHS = (8, 31, 32, 33, 63, 64)
LAYOUTS = ("secret_major", "party_major")
every_prime = pytest.mark.parametrize("p", WIDE_EDGE_PRIMES, ids=PID)


# ---------------------------------------------------------------- the classes
def miller_rabin(n, rounds=40):
    """n is prime: trial division by the primes up to 13, then Miller-Rabin to those bases and to `rounds` seeded random ones"""
    for q in (2, 3, 5, 7, 11, 13):
        if n % q == 0:
            return n == q
    if n < 2:
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    rng = random.Random(n)
    for a in [2, 3, 5, 7, 11, 13] + [rng.randrange(2, n - 1) for _ in range(rounds)]:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_every_member_is_prime_and_every_class_reaches_the_branch_it_names():
    assert len(WIDE_EDGE_PRIMES) == 24 == sum(len(c) for c in WIDE_PRIME_CLASSES.values())
    assert WIDE_SECP_N == SECP_N
    for p in WIDE_EDGE_PRIMES:
        assert miller_rabin(p), hex(p)
    assert not miller_rabin(COMPOSITE_255) and not miller_rabin(65535) and not miller_rabin(561) and not miller_rabin(3 * (2**89 - 1))
    C = WIDE_PRIME_CLASSES
    br = {name: [wide_branches(p) for p in c] for name, c in C.items()}
    bits = {name: [p.bit_length() for p in c] for name, c in C.items()}
    # tiny: the narrow digits of the word reduction; 65521 is the last prime below 2^16 and 65537 the first with a 16-bit digit
    assert [b[3] for b in br["tiny"]] == [1, 2, 2, 7, 8, 15]
    assert [b[3] for b in br["word16"]] == [16] and not any(miller_rabin(q) for q in range(65522, 65537))
    assert all(b[3] == 16 for name in ("one_word", "word_edges", "top") for b in br[name])
    # one_word: both word stages; the bit stage is skipped at 64 bits alone
    assert bits["one_word"] == [31, 32, 33, 63, 64]
    assert all(b[0] and b[1] for b in br["one_word"]) and [b[2] for b in br["one_word"]] == [False, False, False, False, True]
    # word_edges: the 128 stage alone up to 128 bits, the 64 stage alone up to 192 bits, neither above; word moves only at 128, 192
    assert bits["word_edges"] == [65, 96, 128, 129, 160, 192, 193, 224]
    assert [b[:2] for b in br["word_edges"]] == [(True, False)] * 3 + [(False, True)] * 3 + [(False, False)] * 2
    assert [b[2] for b in br["word_edges"]] == [False, False, True, False, False, True, False, False]
    # top: no word stage; the sum of two elements carries out of 256 bits for the three 256-bit members (the `top` paths), and the
    # divisor of the reciprocal wraps for three (pn[3] + 1 == 0), not for 2^255 + 95
    assert bits["top"] == [255, 256, 256, 256] and all(not b[0] and not b[1] for b in br["top"])
    assert [2 * (p - 1) >= 1 << 256 for p in C["top"]] == [False, True, True, True]
    assert [b[4] for b in br["top"]] == [True, False, True, True]
    assert not br["top"][0][2] and all(b[2] for b in br["top"][1:])            # 255 bits shift by one bit; 256 bits by none


# ---------------------------------------------------------------- the stand-alone mirrors
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC]
MIRRORS = {
    # name: (source, arguments in front of the primes, the line of success)
    "step": ("shamir_wide.cpp", ["3000"], "SHAMIR_WIDE_OK"),
    "product": ("shamir_wide_mul.cpp", ["3000"], "SHAMIR_WIDE_MUL_OK"),
    "corrected": ("shamir_wide_corrected.cpp", ["350"], "SHAMIR_WIDE_CORRECTED_OK"),
    "erasures": ("shamir_wide_erasures.cpp", [], "SHAMIR_WIDE_ERASURES_OK"),
    "evaluate": ("shamir_wide_evaluate.cpp", [], "SHAMIR_WIDE_EVALUATE_OK"),
    "packed": ("shamir_packed_wide.cpp", ["60"], "SHAMIR_PACKED_WIDE_OK"),
}


@pytest.mark.parametrize("name", list(MIRRORS))
def test_stand_alone_mirror_at_every_prime_under_sanitizers(name):
    """each program is built with the address and undefined-behaviour sanitizers (static runtimes, its own main) and run over all of
    WIDE_EDGE_PRIMES, six primes to a process and the four processes side by side; a prime whose field is too small for a shape
    gets the shapes it can serve, never none"""
    src, head, ok = MIRRORS[name]
    exe = os.path.join(ROOT, "build", "prime_edges_" + os.path.splitext(src)[0])
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "cpp", src), "-o", exe])
    shares = [WIDE_EDGE_PRIMES[k::4] for k in range(4)]
    assert sorted(p for share in shares for p in share) == WIDE_EDGE_PRIMES
    runs = [subprocess.Popen([exe] + head + [f"{p:x}" for p in share], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for share in shares]
    try:
        for run in runs:
            stdout, stderr = run.communicate(timeout=600)
            assert run.returncode == 0 and ok in stdout, stdout[-3000:] + stderr[-3000:]
    finally:
        for run in runs:
            run.kill()


@pytest.mark.parametrize("holders", [[0, 1], [0, 2, 3, 1], [0, 2, 3, 5, 4], None], ids=["p3", "p5", "p7", "from11"])
def test_handover_mirror_at_every_prime_under_sanitizers(holders):
    """the handover's kernel sequence prints what the kernels would store, compared with the _host routines; its five holders reach
    the point 10, so 3, 5 and 7 bring their own"""
    primes = [p for p in WIDE_EDGE_PRIMES if p > 10] if holders is None else [max(holders) + 2]
    assert primes and (holders is not None or len(primes) == 21)
    args = [] if holders is None else ["holders=" + ",".join(map(str, holders))]
    out = subprocess.run([build_kernel_sequence()] + args + [f"{p:x}" for p in primes], capture_output=True, text=True, timeout=600)
    compare_kernel_sequence(out, primes, holders or [0, 2, 3, 5, 9])


# ---------------------------------------------------------------- dealing
@functools.lru_cache(maxsize=None)
def context(n):
    return params(n)


def dealing_shape(p, pack=1):
    """(n, pack, degrees): n = min(9, p - pack) parties, so that n + pack - 1 < p, with the pack cut down until degree + pack <= n
    leaves a degree; the degrees 0, 1 and the largest one"""
    for K in range(pack, 0, -1):
        n = min(9, p - K)
        if n >= max(K, 2):
            return n, K, sorted({0, min(1, n - K), n - K})
    raise AssertionError(p)


def dealing_case(p, n, K, t, D):
    """(secrets [D][K], explicit coefficients [D][t], seeds): 0, p - 1, p and 2^256 - 1 go round the secrets and the coefficients"""
    rng = random.Random((p & 0xFFFFFF) * 31 + 7 * t + K)
    fixed = [0, p - 1, p, W256]
    secrets = [[fixed[(d + j + t) % 4] for j in range(K)] for d in range(D)]
    coeffs = [[fixed[(d + j + 1) % 4] if j < 4 else rng.getrandbits(256) for j in range(t)] for d in range(D)]
    return secrets, coeffs, seeds_for(D, tag=t + K)


def dealing_expected(p, n, K, secrets, coeffs, seeds, t):
    """([D][n] ints for the explicit coefficients, the same for the drawn ones)"""
    at = (lambda s, c: evaluate(s[0], c, n, p)) if K == 1 else (lambda s, c: packed_evaluate(s, c, n, p))
    return ([at(secrets[d], coeffs[d]) for d in range(len(secrets))],
            [at(secrets[d], restated_coeffs(seeds[d], t, p)) for d in range(len(secrets))])


@every_prime
def test_host_dealing_equals_big_integer_evaluation(p):
    seen = set()
    for pack in (1, 3):
        n, K, degrees = dealing_shape(p, pack)
        assert n + K - 1 < p and (K == pack or p < 10)
        for t in degrees:
            secrets, coeffs, seeds = dealing_case(p, n, K, t, 4)
            seen |= {v for row in secrets + coeffs for v in row}
            explicit, drawn = dealing_expected(p, n, K, secrets, coeffs, seeds, t)
            if K == 1:
                flat = [row[0] for row in secrets]
                assert ints(P.shamir_shares_wide(context(n), flat, t, p, coeffs=coeffs, host=True)) == explicit, ("explicit", t)
                assert ints(P.shamir_shares_wide(context(n), flat, t, p, seeds=seeds, host=True)) == drawn, ("drawn", t)
            call = lambda **kw: ints(P.shamir_shares_packed_wide(context(n), secrets, K, t, p, host=True, **kw))
            assert call(coeffs=coeffs) == explicit, ("packed explicit", K, t)
            assert call(seeds=seeds) == drawn, ("packed drawn", K, t)
    assert {0, p - 1, p, W256} <= seen


# ---------------------------------------------------------------- limbs
def limb_case(p, limb_bits, count):
    """(planes [NL][count] of any 64-bit words, 2^64 - 1 among them and a whole element of them, and what they fold to)"""
    nl = -(-p.bit_length() // limb_bits)
    rng = random.Random((p & 0xFFFFFF) + limb_bits)
    planes = [[rng.getrandbits(64) for _ in range(count)] for _ in range(nl)]
    planes[0][0] = planes[nl - 1][count - 1] = U64
    for w in range(nl):
        planes[w][count // 2] = U64
    want = [sum(planes[w][i] << (w * limb_bits) for w in range(nl)) % p for i in range(count)]
    return nl, np.array(planes, dtype=np.uint64), want


@every_prime
def test_limb_helpers_and_the_fold_of_limb_sums(p):
    rng = random.Random(p & 0xFFFF)
    for lb in LIMB_WIDTHS:
        nl, planes, want = limb_case(p, lb, 9)
        assert nl <= 16 and P.shamir_wide_limbs(p, lb) == nl == P.shamir_wide_handover_shape(p, lb, 64)[0]
        values = [0, p - 1, p // 2] + [rng.randrange(p) for _ in range(6)]
        limbs = P.shamir_wide_to_limbs(values, lb, plain_modulus=p)
        assert limbs.tolist() == [[(v >> (w * lb)) & ((1 << lb) - 1) for v in values] for w in range(nl)]
        assert P.shamir_wide_from_limbs(limbs, p, lb) == values
        assert P.shamir_wide_from_limbs(planes, p, lb) == want


# ---------------------------------------------------------------- the receiving end
def receiving_shape(p):
    """(count, degree): min(12, p - 1) shares and degree 3, cut down where the field is small so that r = count - degree - 1 stays
    at least 1 (p = 3: two shares of degree 0; p = 5: four of degree 1; p = 7: six of degree 3)"""
    count = min(12, p - 1)
    return count, 3 if count >= 6 else 1 if count >= 4 else 0


def edge_indices(rng, count, p):
    """`count` party indices with distinct points below p: the largest legal one (its point is p - 1, or 2^64 above that), 0, and
    random ones; every point of the field where it has no more than `count`"""
    if p - 1 <= count:
        idx = list(range(p - 1))
        rng.shuffle(idx)
        return idx
    idx = [min(p - 2, U64), 0]
    while len(idx) < count:
        i = rng.randrange(1, min(p - 2, 1 << 20))
        if i not in idx:
            idx.append(i)
    return idx


def poly_at(co, x, p):
    v = 0
    for c in reversed(co):
        v = (v * x + c) % p
    return v


def raised(rng, v, p, most=False):
    """a word that reads v mod p: v plus a multiple of p (the largest one with most=True), below 2^256"""
    k = (W256 - v) // p
    return v + p * (k if most else rng.randrange(k + 1))


class Receiving:
    """S = 3 polynomials of degree t over p, dealt in integers at the points of `count` indices, and five targets: the largest
    legal index, three of the columns (the first, the middle one, the last: the scenarios put an error on the first and erase the
    last) and an index that is no column's where the field has one"""

    def __init__(self, p):
        self.p, self.S = p, 3
        self.count, self.t = receiving_shape(p)
        self.r = self.count - self.t - 1
        rng = self.rng = random.Random(p & 0xFFFFFF)
        self.idx = edge_indices(rng, self.count, p)
        self.polys = [[rng.randrange(p) for _ in range(self.t + 1)] for _ in range(self.S)]
        self.polys[0][0], self.polys[1][0], self.polys[2][self.t] = p - 1, 0, p - 1
        self.secrets = [co[0] for co in self.polys]
        self.clean = [[poly_at(co, i + 1, p) for i in self.idx] for co in self.polys]
        off = self.idx[0]
        if p - 1 > self.count:
            off = next(i for i in range(min(p - 2, (1 << 20) + 77), 0, -1) if i not in self.idx)
        self.targets = [min(p - 2, U64), self.idx[0], self.idx[self.count // 2], self.idx[self.count - 1], off]
        self.values = [[poly_at(co, i + 1, p) for i in self.targets] for co in self.polys]

    def held(self, wrong):
        """the rows with the columns wrong[s] of row s deviating, every second word raised by a multiple of p and the first
        raised as far as 256 bits allow"""
        rng, p = self.rng, self.p
        rows = [[(v + 1 + rng.randrange(p - 1)) % p if c in wrong[s] else v for c, v in enumerate(row)] for s, row in enumerate(self.clean)]
        return [[raised(rng, v, p, most=(s, c) == (0, 0)) if (s + c) % 2 == 0 else v for c, v in enumerate(row)] for s, row in enumerate(rows)]

    def checked_scenarios(self):
        """(name, rows, bad, col_bad): a clean matrix, then deviations in the extra columns (beyond the first t + 1), which the
        checked call counts while the secrets stay right"""
        t, count, S = self.t, self.count, self.S
        wrong = [set(), {count - 1}, {t + 1, count - 1} if self.r >= 2 else {count - 1}]
        out = [("clean", self.held([set()] * S), [0] * S, [0] * count)]
        out.append(("extras", self.held(wrong), [len(w) for w in wrong], [sum(c in w for w in wrong) for c in range(count)]))
        return out

    def scenarios(self):
        """(name, rows, erased matrix [S][count] or None, (secrets, nerr, col_err, bits), values) of the corrected and erasure
        calls: clean; row s with min(s, E) errors, row 1's on column 0; the last column flagged (junk in it) with the errors the
        rest of the redundancy corrects; the last two columns flagged.  A row with more flags than r is undecodable"""
        count, S, r, rng = self.count, self.S, self.r, self.rng
        out = []
        for name, flagged in (("clean", None), ("errors", []), ("one_flag", [count - 1]), ("two_flags", [count - 2, count - 1])):
            eps = len(flagged or [])
            budget = 0 if name == "clean" or eps > r else (r - eps) // 2
            free = [c for c in range(1, count) if c not in (flagged or [])]
            wrong = [set(), {0} if budget else set(), set(rng.sample(free, min(budget, len(free))))]
            rows = self.held(wrong)
            erased = None
            if flagged is not None and name != "errors":
                erased = [[c in flagged for c in range(count)] for _ in range(S)]
                for s in range(S):
                    for k, c in enumerate(flagged):
                        rows[s][c] = (W256, 0, rng.getrandbits(256))[(s + k) % 3]
            if eps > r:
                report = ([0] * S, [UNDECODABLE] * S, [0] * count, set())
                values = [[0] * len(self.targets) for _ in range(S)]
            else:
                report = (self.secrets, [len(w) for w in wrong], [sum(c in w for w in wrong) for c in range(count)],
                          {(s, c) for s, w in enumerate(wrong) for c in w})
                values = self.values
            out.append((name, rows, erased, report, values))
        return out


def in_layout(matrix, layout):
    return matrix if layout == "secret_major" else [list(col) for col in zip(*matrix)]


def mask_bits(mask):
    return {(s, c) for s in range(mask.shape[0]) for c in range(64 * mask.shape[1]) if (int(mask[s][c // 64]) >> (c % 64)) & 1}


def host_checked(case, rows, layout):
    out, bad, col_bad = P.shamir_reconstruct_wide_checked(None, case.idx, in_layout(rows, layout), case.t, case.p, host=True, layout=layout)
    return out, bad.tolist(), col_bad.tolist()


def host_decode(case, rows, erased, layout):
    er = None if erased is None else in_layout(erased, layout)
    out, nerr, col_err, mask = P.shamir_reconstruct_wide_corrected(None, case.idx, in_layout(rows, layout), case.t, case.p, host=True,
                                                                   layout=layout, erased=er)
    return out, nerr.tolist(), col_err.tolist(), mask_bits(mask)


def host_evaluate(case, rows, erased, layout):
    er = None if erased is None else in_layout(erased, layout)
    values, out, nerr, col_err, mask = P.shamir_evaluate_wide_corrected(None, case.idx, in_layout(rows, layout), case.t, case.p, case.targets,
                                                                        host=True, layout=layout, erased=er)
    return values, (out, nerr.tolist(), col_err.tolist(), mask_bits(mask))


@every_prime
def test_host_receiving_end_on_sharings_dealt_in_integers(p):
    case = Receiving(p)
    assert case.r >= 1 and len(set(case.idx)) == case.count and all(i + 1 < p for i in case.idx + case.targets)
    assert (p - 1 in [i + 1 for i in case.targets]) == (p - 2 <= U64)
    for name, rows, bad, col_bad in case.checked_scenarios():
        for layout in LAYOUTS:
            assert host_checked(case, rows, layout) == (case.secrets, bad, col_bad), ("checked", name, layout)
    seen = set()
    for name, rows, erased, report, values in case.scenarios():
        seen.add(report[1][0] == UNDECODABLE)
        for layout in LAYOUTS:
            assert host_decode(case, rows, erased, layout) == report, ("decode", name, layout)
            assert host_evaluate(case, rows, erased, layout) == (values, report), ("evaluate", name, layout)
    assert seen == ({False, True} if p == 3 else {False})              # two flags are more than r = 1 leaves at p = 3 only


# ---------------------------------------------------------------- the handover's public arithmetic
def digit_values(p, b, count=65):
    """`count` words of any size: the edges of the signed-digit chain, then random ones"""
    rng = random.Random((p & 0xFFFFFF) + b)
    B = 1 << b
    vals = edge_set(p, b) + [(p // 2 + rng.randrange(-B, B)) % (1 << 256) for _ in range(8)]
    return (vals + [rng.getrandbits(256) for _ in range(count)])[:count]


def weights_case(p):
    """(indices, valid, points): min(5, p - 1) holders with the second masked out, and the points 0, p - 1 and a holder's"""
    D = min(5, p - 1)
    rng = random.Random(p & 0xFFFFF)
    idx = rng.sample(range(min(p - 2, 200)), D) if min(p - 2, 200) >= D else rng.sample(range(p - 1), D)
    return idx, [int(d != 1) for d in range(D)], [0, p - 1, idx[D - 1] + 1]


def fold_case(p, b, count=70, ww=2):
    """(wide [count][V][ww], status [count][V], values, status out) of the fold of the digit plaintexts"""
    V = num_digits(p, b)
    rng = random.Random((p & 0xFFFFFF) * 3 + b)
    wide = np.array([[[rng.getrandbits(64) for _ in range(ww)] for _ in range(V)] for _ in range(count)], dtype=np.uint64)
    status = np.array([[rng.choice([0, 1, 2, 3, 4, 6, 7]) for _ in range(V)] for _ in range(count)], dtype=np.uint32)
    wide[0] = 0
    status[0, 0] = P.DEC_NEGATIVE
    wide[1, :, 1:] = 0
    wide[2] = U64
    vals, st = fold_ref(p, b, wide.tolist(), status.tolist())
    return wide, status, vals, st


@every_prime
def test_host_handover_arithmetic_against_python_integers(p):
    idx, valid, points = weights_case(p)
    assert all(i + 1 < p for i in idx) and len(set(idx)) == len(idx)
    for b in DIGIT_WIDTHS:
        V, B = num_digits(p, b), 1 << b
        assert V <= 33 and P.shamir_wide_handover_shape(p, 52, b)[1] == V
        vals = digit_values(p, b)
        got = P.shamir_wide_signed_digits(None, vals, p, b, host=True)
        assert got.shape == (65, V) and got.tolist() == [digits_ref(x, p, b) for x in vals], b
        assert all(-(B // 2) <= c < B // 2 for row in got.tolist() for c in row), b
        for lb in (52, 62):
            got = P.shamir_wide_handover_weights(None, idx, p, valid, points, lb, b, host=True)
            assert got.tolist() == weights_ref(p, idx, valid, points, lb, b), (b, lb)
        wide, status, want, wst = fold_case(p, b, 9)
        vals, st = P.shamir_wide_from_digits(None, wide, status, p, b, host=True)
        assert vals == want and st.tolist() == wst, b

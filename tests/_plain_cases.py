"""Inputs and the restated contract of the plain decode, shared by tests/test_plain_decode_host.py and the GPU
worker tests/_plain_decode_worker.py.  P is the model's plaintext before the u64 conversion (oracle/pvw_model.py's
decode_scalar_pvw up to that line, restated in tests/test_checked_decode_host.py as plain_of); from it the contract is plain
integer arithmetic: out = P mod p, the words of |P|, the three status bits, and the noise of DESIGN 8.6."""
import numpy as np

import pvw_model as M
import test_checked_decode_host as TC
from _util import primes_1mod

U64 = (1 << 64) - 1
DEC_LOSSY, DEC_NEGATIVE, DEC_WIDE_TRUNCATED = 1, 2, 4

# the seven sets of the checked decode's test plus 17 x 61-bit at l = 8 (the config-3 chain)
SETS = dict(TC.SETS, bench17_l8=(M.bench_moduli(17), 8))
FIXED_MODULI = [2, 3, 1 << 32, 1 << 61, (1 << 61) - 1, (1 << 62) - 57]


def moduli_for(set_moduli):
    """2, 3, 2^32, 2^61, 2^61 - 1, 2^62 - 57 and the set's own first limb"""
    return FIXED_MODULI + [int(set_moduli[0])]


def q_words(m):
    return (m.Q.bit_length() + 63) // 64


def radius(m):
    """the decoding radius pvw_ctx_sum_capacity describes: the largest R with R (Delta^(l-1) + 1) < Q / 2 (Q odd)"""
    return (m.Q - 1) // (2 * (m.delta_power_l_minus_1 + 1))


def chosen(m):
    """(P, noise vector) pairs: the plaintexts the issue lists, each with noise vectors inside the radius"""
    Q, l = m.Q, m.l
    rng = np.random.default_rng(1000 * l + len(m.moduli))
    big = lambda bits: int.from_bytes(rng.bytes((bits + 7) // 8), "little") >> ((-bits) % 8)
    half = Q // 2
    plains = [0, 1, -1, -1000, -1001, 1 << 63, U64, 1 << 64, (1 << 64) + 1, big(75), big(75) | (1 << 74),
              big(Q.bit_length() + 8) % Q - half, -(big(Q.bit_length() + 8) % half), half]
    R = radius(m)
    small = min(R, 10 ** 6)
    out = []
    for pl in plains:
        vecs = [[0] * l, [int(x) for x in rng.integers(-small, small + 1, size=l)], [R] * l, [-R] * l,
                [R if j % 2 else -R for j in range(l)]]
        e = [0] * l
        e[int(rng.integers(0, l))] = R
        vecs.append(e)
        out += [(pl, v) for v in vecs]
    return out


def chosen_cases(m):
    Q, D = m.Q, m.delta
    return [[(-(pl * D ** j) + e[j]) % Q for j in range(m.l)] for pl, e in chosen(m)]


def uniform_cases(m, count=48):
    rng = np.random.default_rng(55 + m.l)
    nb = (m.Q.bit_length() + 71) // 8
    return [[int.from_bytes(rng.bytes(nb), "little") % m.Q for _ in range(m.l)] for _ in range(count)]


def all_cases(m):
    """the checked decode's boundary inputs, the chosen plaintexts, uniform residues (garbage in: the definition still holds)"""
    return TC.checked_cases(m) + chosen_cases(m) + uniform_cases(m)


def rns(cases, moduli):
    return TC._rns(cases, moduli)


def unreduce(noisy, moduli):
    """w + j q for the largest j that stays below 2^64: the same residues as unreduced input words"""
    big = noisy.copy()
    for i, q in enumerate(moduli):
        j = (U64 - big[:, i, :].astype(object)) // q
        big[:, i, :] = (big[:, i, :].astype(object) + j * q).astype(np.uint64)
    return big


def contract(z_ints, m, modulus, wide_words):
    """(out, noise, status, wide words) of one input by the contract of DESIGN 8.8"""
    Q, D = m.Q, m.delta
    p = TC.plain_of(z_ints, m)
    noise = min(max(abs(M.center((-z_ints[i] - p * D ** i) % Q, Q)) for i in range(m.l)), U64)
    status = 0 if 0 <= p <= U64 else DEC_LOSSY
    if modulus or wide_words:
        status |= DEC_NEGATIVE if p < 0 else 0
        if wide_words and abs(p) >> (64 * wide_words):
            status |= DEC_WIDE_TRUNCATED
    out = p % modulus if modulus else M.decode_scalar_pvw(z_ints, m)
    wide = [(abs(p) >> (64 * w)) & U64 for w in range(wide_words)]
    return out, noise, status, wide


def contract_arrays(cases, m, modulus, wide_words):
    rows = [contract(z, m, modulus, wide_words) for z in cases]
    return (np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.uint64),
            np.array([r[2] for r in rows], dtype=np.uint32),
            np.array([r[3] for r in rows], dtype=np.uint64).reshape(len(rows), wide_words))


def option_grid(m):
    """(modulus, wide_words) pairs every comparison runs: each modulus with every word of Q, the first limb with one and
    two words (truncation), the wide integer alone"""
    W = q_words(m)
    grid = [(p, W) for p in moduli_for(m.moduli)]
    grid += [(int(m.moduli[0]), w) for w in (1, 2) if w <= W] + [(0, W), ((1 << 61) - 1, 0)]
    return grid

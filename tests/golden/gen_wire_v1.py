"""Writes tests/golden/wire_v1_params.bin and wire_v1_ciphertext.bin: wire-format version 1 blobs made from the
specification alone (no library call), which the version-1 reader must keep accepting.  Run from the repository root:
python tests/golden/gen_wire_v1.py"""
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# n, k, l, moduli (36/37-bit chain of the reference's tests), variance, bounds
N, K, ELL = 3, 2, 8
MODULI = [0xFFFFEE001, 0xFFFFC4001, 0x1FFFFE0001]
VARIANCE, B1, B2 = 0.5, 100, 200
C1, C2 = (0, K), (1, 3)                  # c1 rows [0, 2), c2 rows [1, 3)


def words():
    """the ciphertext rows the fixture holds: [polys][L][l], residues below q_i"""
    rng = np.random.default_rng(20261016)
    count = (C1[1] - C1[0]) + (C2[1] - C2[0])
    return [[[int(rng.integers(0, q)) for _ in range(ELL)] for q in MODULI] for _ in range(count)]


def header(kind, ranges, body_len):
    h = b"PVWw" + struct.pack("<HHI", 1, kind, 0) + struct.pack("<IIII", N, K, ELL, len(MODULI))
    h += struct.pack("<fQQ", VARIANCE, B1, B2) + struct.pack(f"<{len(MODULI)}Q", *MODULI)
    h += b"".join(struct.pack("<II", lo, hi) for lo, hi in ranges) + struct.pack("<Q", body_len)
    return h + bytes(-len(h) % 16)


def pack(polys):
    out = b""
    for poly in polys:
        for row, q in zip(poly, MODULI):
            w = q.bit_length()
            out += sum(v << (j * w) for j, v in enumerate(row)).to_bytes(ELL * w // 8, "little")
    return out


if __name__ == "__main__":
    body = pack(words())
    with open(os.path.join(HERE, "wire_v1_params.bin"), "wb") as f:
        f.write(header(1, [], 0))
    with open(os.path.join(HERE, "wire_v1_ciphertext.bin"), "wb") as f:
        f.write(header(4, [C1, C2], len(body)) + body)

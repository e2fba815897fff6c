"""Wire format version 1 on the host: the specification restated here in Python -- header fields, and a packed
polynomial as L rows of l residues at bitlen(q_i) bits each, least significant bit first, little-endian -- against the
library's plain C++ codec (pvw_wire_pack_host / pvw_wire_unpack_host), its header writer and checker, the parameter and
secret-key blobs, and the committed version-1 fixtures.  No GPU."""
import os
import re
import struct

import numpy as np
import pytest

import pvw_rs_amd as P
from pvw_rs_amd import _ffi, api
from _util import EXAMPLE_MODULI, TEST_MODULI, primes_1mod
from pvw_rs_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U64 = (1 << 64) - 1


# ---- the specification, restated -----------------------------------------------------------------------------------
def spec_poly_bytes(moduli, l):
    return l // 8 * sum(q.bit_length() for q in moduli)


def spec_pack(polys, moduli, l):
    out = bytearray()
    for poly in polys:
        for row, q in zip(poly, moduli):
            w = q.bit_length()
            out += sum((int(v) % q) << (j * w) for j, v in enumerate(row)).to_bytes(l * w // 8, "little")
    return bytes(out)


def spec_fields(data, count, moduli, l):
    """the raw fields, [count][L][l] Python ints"""
    out, o = [], 0
    for _ in range(count):
        poly = []
        for q in moduli:
            w = q.bit_length()
            nb = l * w // 8
            row = int.from_bytes(data[o:o + nb], "little")
            o += nb
            poly.append([(row >> (j * w)) & ((1 << w) - 1) for j in range(l)])
        out.append(poly)
    return out


def spec_header(kind, repr, n, k, l, moduli, variance, b1, b2, roots=None, ranges=(), body_len=0):
    h = b"PVWw" + struct.pack("<HHI", 1, kind, repr) + struct.pack("<IIII", n, k, l, len(moduli))
    h += struct.pack("<fQQ", variance, b1, b2) + struct.pack(f"<{len(moduli)}Q", *moduli)
    if roots is not None:
        h += struct.pack(f"<{len(roots)}Q", *roots)
    h += b"".join(struct.pack("<II", lo, hi) for lo, hi in ranges) + struct.pack("<Q", body_len)
    return h + bytes(-len(h) % 16)


# ---- chains ------------------------------------------------------------------------------------------------------------
def chains(l):
    m = 2 * l
    tiny = primes_1mod(m, 2, top=max(256, 16 * m))
    c40 = primes_1mod(128, 2, top=1 << 40)
    c61 = W.bench_moduli(5) if l <= 32 else primes_1mod(128, 5)      # the bench chain is 1 mod 64
    c62 = primes_1mod(128, 2, top=1 << 62)
    out = {"tiny": tiny, "40": c40, "56": EXAMPLE_MODULI, "61": c61, "62": c62,
           "mixed": [c62[0], tiny[0], c40[0], EXAMPLE_MODULI[0], c61[0]]}
    if l <= 32:
        out["36/37"] = TEST_MODULI
    return out


def params(moduli, l, n=3, k=2, **kw):
    b = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli)
    for name, v in kw.items():
        b = getattr(b, name)(*v) if isinstance(v, tuple) else getattr(b, name)(v)
    return b.build()


def words(rng, count, moduli, l, unreduced=False):
    a = np.empty((count, len(moduli), l), dtype=np.uint64)
    for i, q in enumerate(moduli):
        if unreduced:
            a[:, i, :] = rng.integers(0, 1 << 64, size=(count, l), dtype=np.uint64)
        else:
            a[:, i, :] = rng.integers(0, q, size=(count, l), dtype=np.uint64)
    # edge words on limb 0 of the first polynomial: 0, q-1 (and, unreduced, q, 2^64-1)
    q = moduli[0]
    a[0, 0, :4] = [0, q - 1, q if unreduced else 1, U64 if unreduced else q // 2]
    return a


def reduce(a, moduli):
    return np.stack([a[:, i, :] % np.uint64(q) for i, q in enumerate(moduli)], axis=1)


@pytest.mark.parametrize("l", [8, 16, 32, 64])
def test_host_pack_matches_the_specification(l):
    rng = np.random.default_rng(l)
    for name, moduli in chains(l).items():
        p = params(moduli, l)
        assert p.wire_poly_bytes() == spec_poly_bytes(moduli, l), name
        for count in (1, 15, 16, 17, 300 if l <= 16 else 40):
            a = words(rng, count, moduli, l)
            got = api.wire_pack_host(p, a)
            assert got == spec_pack(a, moduli, l), (name, l, count)
            assert np.array_equal(api.wire_unpack_host(p, got, count), a), (name, l, count)


@pytest.mark.parametrize("l", [8, 64])
def test_unreduced_words_pack_as_their_residues(l):
    rng = np.random.default_rng(100 + l)
    for name, moduli in chains(l).items():
        p = params(moduli, l)
        a = words(rng, 17, moduli, l, unreduced=True)
        r = reduce(a, moduli)
        got = api.wire_pack_host(p, a)
        assert got == api.wire_pack_host(p, r) == spec_pack(r, moduli, l), name
        assert np.array_equal(api.wire_unpack_host(p, got, 17), r), name


def _corrupt(data, moduli, l, poly, limb, slot, field):
    """`data` with the field of (poly, limb, slot) replaced"""
    pb = spec_poly_bytes(moduli, l)
    off = poly * pb + l // 8 * sum(q.bit_length() for q in moduli[:limb])
    w = moduli[limb].bit_length()
    nb = l * w // 8
    row = int.from_bytes(data[off:off + nb], "little")
    row = (row & ~(((1 << w) - 1) << (slot * w))) | (field << (slot * w))
    return data[:off] + row.to_bytes(nb, "little") + data[off + nb:]


@pytest.mark.parametrize("l", [8, 32])
def test_out_of_range_fields_are_rejected_with_their_index(l):
    rng = np.random.default_rng(7 * l)
    for name, moduli in chains(l).items():
        p = params(moduli, l)
        a = words(rng, 20, moduli, l)
        good = api.wire_pack_host(p, a)
        limb = len(moduli) - 1
        q, w = moduli[limb], moduli[limb].bit_length()
        old = int(a[13, limb, 5])
        for field in (q, (1 << w) - 1, old | (1 << (w - 1)) if old | (1 << (w - 1)) >= q else (1 << w) - 2):
            bad = _corrupt(good, moduli, l, 13, limb, 5, field)
            assert spec_fields(bad, 20, moduli, l)[13][limb][5] == field
            with pytest.raises(P.PvwError) as e:
                api.wire_unpack_host(p, bad, 20)
            assert e.value.variant == "DeserializationError", name
            assert re.search(rf"polynomial 13, limb {limb}, slot 5\b", str(e.value)), str(e.value)
        # two bad fields: both counted, the first one named
        twice = _corrupt(_corrupt(good, moduli, l, 4, 0, 0, moduli[0]), moduli, l, 19, limb, l - 1, q)
        import ctypes as C
        out = np.zeros((20, len(moduli), l), dtype=np.uint64)
        buf = np.frombuffer(twice, dtype=np.uint8)
        cnt = C.c_uint64()
        rc = p._lib.pvw_wire_unpack_host(p._h, buf.ctypes.data_as(C.c_void_p), 20, out.ctypes.data_as(C.c_void_p), C.byref(cnt))
        assert rc == 8 and cnt.value == 2 and "polynomial 4, limb 0, slot 0" in _ffi.last_error(p._lib)


def test_header_round_trip_and_layout():
    moduli = TEST_MODULI
    p = params(moduli, 8, n=5, k=3, set_secret_variance=0.75, set_error_bounds=(11, 22))
    pb = spec_poly_bytes(moduli, 8)
    cases = [(_ffi.WIRE_PARAMS, P.REPR_POWER, (), 0), (_ffi.WIRE_SK, P.REPR_POWER, (), 3 * 8 * 8),
             (_ffi.WIRE_CRS, P.REPR_POWER, ((1, 3),), 2 * 3 * pb), (_ffi.WIRE_PK, P.REPR_NTT, ((0, 5),), 5 * 3 * pb),
             (_ffi.WIRE_CT, P.REPR_NTT, ((0, 3), (2, 4)), 5 * pb)]
    for kind, repr, ranges, body_len in cases:
        flat = [x for r in ranges for x in r] + [0] * (4 - 2 * len(ranges))
        head = api._wire_header(p, kind, repr, *flat).tobytes()
        roots = p.roots() if repr == P.REPR_NTT else None
        assert head == spec_header(kind, repr, 5, 3, 8, moduli, 0.75, 11, 22, roots, ranges, body_len), kind
        assert len(head) % 16 == 0
        blob = head + bytes(range(256)) * (body_len // 256) + bytes(body_len % 256)
        if kind in (_ffi.WIRE_CRS, _ffi.WIRE_PK, _ffi.WIRE_CT):
            blob = head + api.wire_pack_host(p, np.zeros((body_len // pb, 3, 8), dtype=np.uint64))
        got = api._wire_check(p, blob, kind)
        assert got[0] == repr and got[1] == tuple(flat) and got[2] == len(head)


def _err(fn):
    with pytest.raises(P.PvwError) as e:
        fn()
    return e.value.variant


def test_header_rejections():
    p = params(TEST_MODULI, 8)
    blob = p.to_bytes()
    ok = lambda b: api._wire_check(p, b, _ffi.WIRE_PARAMS)   # noqa: E731
    ok(blob)
    assert _err(lambda: ok(b"XVWw" + blob[4:])) == "InvalidFormat"                       # magic
    assert _err(lambda: ok(blob[:4] + struct.pack("<H", 2) + blob[6:])) == "InvalidFormat"   # version
    assert _err(lambda: ok(blob[:6] + struct.pack("<H", 9) + blob[8:])) == "InvalidFormat"   # unknown kind
    assert _err(lambda: ok(blob[:6] + struct.pack("<H", 4) + blob[8:])) == "InvalidFormat"   # body_len of another kind
    assert _err(lambda: ok(blob[:-1])) == "InvalidFormat"                                     # truncated
    assert _err(lambda: ok(blob[:20])) == "InvalidFormat"
    assert _err(lambda: ok(b"")) == "InvalidFormat"
    assert _err(lambda: ok(blob + b"\0")) == "InvalidFormat"                                  # trailing bytes
    assert _err(lambda: ok(blob[:-1] + b"\1")) == "InvalidFormat"                             # padding not zero
    # a blob for other parameters
    for other, want in ((params(TEST_MODULI, 8, n=4), "DimensionMismatch"), (params(TEST_MODULI, 8, k=3), "DimensionMismatch"),
                        (params(TEST_MODULI, 16), "DimensionMismatch"), (params(TEST_MODULI[:2], 8), "DimensionMismatch"),
                        (params(EXAMPLE_MODULI[:3], 8), "InvalidFormat"),
                        (params(TEST_MODULI, 8, set_secret_variance=1.0), "InvalidFormat"),
                        (params(TEST_MODULI, 8, set_error_bounds=(100, 201)), "InvalidFormat")):
        assert _err(lambda: api._wire_check(other, blob, _ffi.WIRE_PARAMS)) == want
    # the kind a reader asks for
    assert _err(lambda: P.SecretKey.from_bytes(p, blob)) == "InvalidFormat"
    # NTT-domain bodies carry the roots: a context with other roots rejects them
    head = api._wire_header(p, _ffi.WIRE_CT, P.REPR_NTT, 0, 2, 0, 3).tobytes()
    body = api.wire_pack_host(p, np.zeros((5, 3, 8), dtype=np.uint64))
    api._wire_check(p, head + body, _ffi.WIRE_CT)
    q2 = params(TEST_MODULI, 8)
    q2.set_roots([pow(r, 3, q) for r, q in zip(q2.roots(), TEST_MODULI)])
    assert _err(lambda: api._wire_check(q2, head + body, _ffi.WIRE_CT)) == "InvalidFormat"
    # ... and row ranges beyond the parameters
    assert _err(lambda: api._wire_header(p, _ffi.WIRE_PK, P.REPR_POWER, 0, 4)) == "InvalidFormat"
    bad = spec_header(_ffi.WIRE_CT, 0, 3, 2, 8, TEST_MODULI, 0.5, 100, 200, None, ((0, 3), (0, 3)), 6 * spec_poly_bytes(TEST_MODULI, 8))
    assert _err(lambda: api._wire_check(p, bad + bytes(6 * spec_poly_bytes(TEST_MODULI, 8)), _ffi.WIRE_CT)) == "InvalidFormat"


def test_parameters_and_secret_keys_round_trip():
    for moduli, l in ((TEST_MODULI, 8), (EXAMPLE_MODULI, 16), (W.bench_moduli(17), 8)):
        p = params(moduli, l, n=7, k=4, set_secret_variance=1.5, set_error_bounds=(123, 4567))
        blob = p.to_bytes()
        q = P.PvwParameters.from_bytes(blob)
        assert (q.n, q.k, q.l, q.moduli(), q.secret_variance, q.error_bound_1, q.error_bound_2) == \
            (7, 4, l, list(moduli), 1.5, 123, 4567)
        assert q.to_bytes() == blob
        coeffs = np.random.default_rng(l).integers(-3, 4, size=(4, l), dtype=np.int64)
        coeffs[0, 0] = -(1 << 63)
        coeffs[0, 1] = (1 << 63) - 1
        sk = P.SecretKey.from_coefficients(p, coeffs)
        sb = sk.to_bytes()
        assert isinstance(sb, bytearray) and len(sb) == len(api._wire_header(p, _ffi.WIRE_SK)) + 4 * l * 8
        assert bytes(sb[-4 * l * 8:]) == coeffs.astype("<i8").tobytes()
        back = P.SecretKey.from_bytes(q, sb)
        assert np.array_equal(back.secret_coeffs, coeffs)
        sb[:] = bytes(len(sb))
    with pytest.raises(P.PvwError):
        P.PvwParameters.from_bytes(b"PVWw" + bytes(60))


def test_poly_bytes_formula():
    for l in (8, 16, 32, 64):
        for moduli in chains(l).values():
            assert params(moduli, l).wire_poly_bytes() == l // 8 * sum(q.bit_length() for q in moduli)


def test_version_1_fixtures_are_still_accepted():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_wire_v1", os.path.join(GOLDEN, "gen_wire_v1.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    pblob = open(os.path.join(GOLDEN, "wire_v1_params.bin"), "rb").read()
    cblob = open(os.path.join(GOLDEN, "wire_v1_ciphertext.bin"), "rb").read()
    p = P.PvwParameters.from_bytes(pblob)
    assert (p.n, p.k, p.l, p.moduli(), p.secret_variance, p.error_bound_1, p.error_bound_2) == \
        (gen.N, gen.K, gen.ELL, gen.MODULI, gen.VARIANCE, gen.B1, gen.B2)
    assert p.to_bytes() == pblob
    repr, ranges, hl, _ = api._wire_check(p, cblob, _ffi.WIRE_CT)
    assert repr == P.REPR_POWER and ranges == (*gen.C1, *gen.C2)
    want = np.array(gen.words(), dtype=np.uint64)
    assert np.array_equal(api.wire_unpack_host(p, cblob[hl:], len(want)), want)
    assert api.wire_pack_host(p, want) == cblob[hl:]

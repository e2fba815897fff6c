"""CPU checks of the residue-word contract (include/pvw_hip.h): a word w a caller passes in limb i means w mod q_i.  The
checks of reduce_word (pvw_arith.h) at every unreduced word class, ahead of the l-point NTTs and the balanced digits,
live in tests/cpp/arith_edges.cpp and run with test_modulus_edges_host.py; here the same checker with the words taken
raw must fail, and the kernel sources must reduce caller words before they transform or digitise them."""
import os
import re

import pvw_model as M
from _util import EDGE_MODULI
from test_modulus_edges_host import CSRC, _run_arith


def test_raw_words_without_reduce_word_fail_at_every_width():
    # the same checker with the words going into the transforms and the digits unreduced (what the kernels did before
    # reduce_word): only the raw-word checks fail, and they fail for every class modulus
    moduli = EDGE_MODULI + M.bench_moduli(2)
    out = _run_arith(moduli, "PVW_RAW_WORDS")
    assert out.returncode == 1
    fails = [ln for ln in out.stdout.splitlines() if ln.startswith("FAIL")]
    assert fails and all(ln.split()[1].startswith("raw_words.") for ln in fails), fails[:10]
    failed_q = {int(re.search(r"q=(\d+)", ln).group(1)) for ln in fails}
    assert failed_q == set(moduli), sorted(set(moduli) - failed_q)
    assert {ln.split()[1] for ln in fails} >= {"raw_words.digits", "raw_words.ntt_forward.8", "raw_words.ntt_inverse.8"}


def _bodies():
    """name -> source of every kernel / device function of the library"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"(?:__global__[^{;]*?void|PVW_HD[^{;(]*?|__device__ __forceinline__[^{;(]*?)\s(\w+)\s*\(", src):
            body = src[m.start():]
            out[m.group(1)] = body[:body.find("\n}\n")]
    return out


# kernels that take caller words into an NTT, the balanced digits, a submod or a byte truncation
CALLER_WORD_KERNELS = [
    "ntt_poly_kernel", "ntt_kernel",                           # pvw_ntt_*, power-basis ciphertexts of decrypt
    "tile_kernel", "untile_kernel",                            # power-basis loads, power-basis downloads of NTT loads
    "mftile7_kernel",                                          # 7-byte GEMM operand: drops byte 7
    "vec_digits_kernel", "vec_digits7_kernel",                 # keygen's A-hat columns; any vector launch_vec_digits is given
    "decrypt_mac_kernel", "decrypt_mac_grouped_kernel", "decrypt_mac_fw_kernel", "decrypt_finish_kernel",   # c2
    "gemm_finish_decrypt_kernel",                              # c2 of decrypt_all
    "decode_chain_body", "decode_one_fixed",                   # pvw_decode[_device]
]


def test_every_kernel_on_caller_words_reduces_them_first():
    bodies = _bodies()
    for name in CALLER_WORD_KERNELS:
        assert name in bodies, name
        assert "reduce_word(" in bodies[name], f"{name} takes caller words without reduce_word"
    # and no other kernel runs a transform or the digit form on words that are neither reduced nor signed residues
    for name, body in bodies.items():
        if name in ("ntt_forward", "ntt_inverse", "stage_inverse"):   # the transforms themselves; decrypt's own residues
            continue
        if re.search(r"ntt_(forward|inverse)<|\+ C\) \^ C", body):
            assert "reduce_word(" in body or "signed_residue(" in body, name
    # the reduction happens at the load, ahead of the transform
    for name in ("tile_kernel", "untile_kernel"):
        b = bodies[name]
        assert b.index("reduce_word(") < b.index("ntt_forward<" if name == "tile_kernel" else "ntt_inverse<"), name
    # the 7-byte operand is built from the reduced word; launch_mftile needs the moduli for it
    assert re.search(r"x\[p\] = reduce_word\(", bodies["mftile7_kernel"])
    capi = open(os.path.join(CSRC, "pvw_capi.hip")).read()
    assert capi.count("c->xm_bytes, c->dt.mods)") == 2

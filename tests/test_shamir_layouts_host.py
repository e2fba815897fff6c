"""The scratch layouts and the sizing rules that the Shamir reconstruction entry points of both fields run through (DESIGN
"Reconstruction entry points", pvw_shamir_fields.h): every offset, size and threshold against the formulas that the one-word and
the 256-bit drivers each carried before the fold, as a stand-alone program under sanitizers.  No device is used."""
import os
import subprocess

from test_shamir_wide_host import CSRC, ROOT


def test_layouts_and_sizing_rules_of_both_fields_under_sanitizers():
    """tests/cpp/shamir_layouts.cpp walks count in {1, 2, 7, 64, 65, 4096} x degree in {0, 2, count - 1} x erasures x cap in
    {1, 2, 5} x Tg in {1, 2, 3, 64} for both fields (and three call sizes and three budgets for the sizing rules): the offsets,
    bytes(), m_bytes(), secret_bytes(), correct_piece, evaluate_group, evaluate_piece and evaluate_need_bytes equal the earlier
    formulas, every wide element region starts at a multiple of four words, and evaluate_need_bytes covers the layout of the pass
    it is for.  Nothing sanitized is loaded into Python."""
    exe = os.path.join(ROOT, "build", "shamir_layouts")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "shamir_layouts.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SHAMIR_LAYOUTS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    cases = int(out.stdout.split("cases")[1].split()[0])
    assert cases == 2 * 15 * 2 * 3 * 4 * 3 * 3                        # 15 (count, degree) pairs, both fields

"""bench.py --dump-outputs: the arrays the timed path's last step returned, written as float64 without loss, identical from
run to run, at most 64 MB in all (a fixed, seeded sample of the rows beyond that); and --steps / --warmup are the counts
the result line reports on every path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
LIMIT = 64_000_000


def words(path):
    """DIR/<name>.npy (float64 pairs: high 32 bits, low 32 bits) -> the u64 words"""
    a = np.load(path)
    assert a.dtype == np.float64 and a.shape[-1] == 2
    assert np.all(a == np.floor(a)) and a.min() >= 0 and a.max() < 2 ** 32
    return (a[..., 0].astype(np.uint64) << np.uint64(32)) | a[..., 1].astype(np.uint64)


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def arrays(seed, shapes):
    rng = np.random.default_rng(seed)
    return {name: rng.integers(0, 2 ** 64, size=shape, dtype=np.uint64) for name, shape in shapes.items()}


SMALL = {"c1": (256, 17, 8), "c2": (16, 17, 8), "values": (16,)}
LARGE = {"c1": (256, 34, 16), "c2": (9000, 34, 16)}                # 5.0 M words: 80 MB as float64 pairs

# bench.dump_outputs on host arrays (a child process: importing bench sets HIP runtime variables)
_DUMP = """
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import bench
sys.path.insert(0, sys.argv[2])
from test_bench_outputs import arrays, SMALL, LARGE
for which, shapes in (("small", SMALL), ("large", LARGE)):
    for run in ("a", "b"):
        res = arrays(11, shapes)
        spec = {n: (a.shape[0], a[0].size, lambda idx, a=a: a[idx].view(np.int64)) for n, a in res.items()}
        bench.dump_outputs(f"{sys.argv[3]}/{which}_{run}", spec, 0, 1)
"""


def test_dump_outputs_exact_bounded_and_repeatable(tmp_path):
    r = subprocess.run([sys.executable, "-c", _DUMP, ROOT, os.path.dirname(os.path.abspath(__file__)), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for which, shapes in (("small", SMALL), ("large", LARGE)):
        a_dir, b_dir = tmp_path / f"{which}_a", tmp_path / f"{which}_b"
        assert sorted(os.listdir(a_dir)) == sorted(os.listdir(b_dir))
        for f in os.listdir(a_dir):
            assert (a_dir / f).read_bytes() == (b_dir / f).read_bytes(), f
        assert dir_bytes(a_dir) <= LIMIT
        if which == "large":
            assert dir_bytes(a_dir) > 0.95 * LIMIT            # the sample fills the budget
        for name, want in arrays(11, shapes).items():
            got = words(a_dir / f"{name}.npy")
            sampled = which == "large" and name == "c2"           # the small arrays stay whole beside a large one
            assert (a_dir / f"{name}_rows.npy").exists() == sampled
            if not sampled:
                assert np.array_equal(got, want)
            else:
                rows = np.load(a_dir / f"{name}_rows.npy")
                assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0)
                assert np.array_equal(got, want[rows.astype(np.int64)])


def test_bench_rejects_a_step_count_below_one():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def run_bench(out_dir, *extra):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--no-cpu", "--no-probe", "--sustain-seconds", "0",
                        "--dump-outputs", str(out_dir)] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["ms_per_step"] > 0 and dir_bytes(out_dir) <= LIMIT
    return d


@pytest.mark.gpu
def test_bench_encrypt_dump_is_the_ciphertext_of_its_workload(tmp_path):
    import pvw_rs_amd as P
    from pvw_rs_amd import dist as D
    from pvw_rs_amd import workloads as W
    args = ["--config", "c1", "--steps", "3", "--warmup", "1"]
    d = run_bench(tmp_path / "a", *args)
    run_bench(tmp_path / "b", *args)
    assert d["steps"] == 3 and d["warmup"] == 1
    for f in ("c1.npy", "c2.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    # the same workload through the host-buffer entry point
    n, k, l, L, _ = W.ENCRYPT_CONFIGS["c1"]
    params = D.sharded_builder(n, k, l, W.config_moduli("c1", L), 1, 0, device=0) \
        .set_secret_variance(W.SECRET_VARIANCE).set_error_bounds_u32(W.ERROR_BOUND_1, W.ERROR_BOUND_2).build()
    gpk = P.GlobalPublicKey.new(P.PvwCrs.new_deterministic(params, W.SEED_A))
    gpk.fill_uniform(W.SEED_B)
    ct = P.encrypt(W.scalars(n), gpk, W.SEED_ENC)
    assert np.array_equal(words(tmp_path / "a" / "c1.npy"), ct.c1)
    assert np.array_equal(words(tmp_path / "a" / "c2.npy"), ct.c2)


@pytest.mark.gpu
def test_bench_decrypt_dump_holds_the_dealt_values(tmp_path):
    from pvw_rs_amd import workloads as W
    d = run_bench(tmp_path, "--path", "decrypt", "--config", "c5x16", "--steps", "2", "--warmup", "0")
    D, k, l, L, _ = W.DECRYPT_CONFIGS["c5x16"]
    assert d["steps"] == 2 and d["warmup"] == 0 and d["decrypts_to_the_dealt_values"]
    assert list(words(tmp_path / "values.npy").reshape(-1)) == [dd * 1000 + 1 for dd in range(D)]
    noisy = words(tmp_path / "noisy.npy")
    assert noisy.shape == (D, L, l)
    assert np.all(noisy < np.array(W.bench_moduli(L), dtype=np.uint64)[None, :, None])


@pytest.mark.gpu
def test_bench_keygen_runs_the_steps_asked_for_and_dumps_b_hat(tmp_path):
    from pvw_rs_amd import workloads as W
    d = run_bench(tmp_path, "--path", "keygen", "--config", "c1", "--steps", "7", "--warmup", "0")
    n, k, l, L, _ = W.ENCRYPT_CONFIGS["c1"]
    assert d["steps"] == 7 and d["warmup"] == 0
    b = words(tmp_path / "b_hat.npy")
    assert b.shape == (n, k, L, l) and b.any()
    assert np.all(b < np.array(W.bench_moduli(L), dtype=np.uint64)[None, None, :, None])

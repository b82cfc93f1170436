"""bench.py's own contract: a plain run times exactly --steps steps and prints the headline only (the other legs need --full), and
--dump-outputs writes what the last timed step computed -- checked against the CPU oracle, in one rank and in a grid of two."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gf2util as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("C_sample_rows", "C_sample_row_index", "C_row_parity", "C_col_parity")


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in DUMPED}


def _check_dump(got, c_bits, k):
    idx = got["C_sample_row_index"].astype(np.int64)
    assert got["C_sample_row_index"].dtype == np.float64 and len(idx) == k and np.all(np.diff(idx) > 0)
    for name in ("C_sample_rows", "C_row_parity", "C_col_parity"):
        assert got[name].dtype == np.float32, name
    assert np.array_equal(got["C_sample_rows"], c_bits[idx].astype(np.float32))
    assert np.array_equal(got["C_row_parity"], (c_bits.sum(axis=1) % 2).astype(np.float32))
    assert np.array_equal(got["C_col_parity"], (c_bits.sum(axis=0) % 2).astype(np.float32))


@pytest.mark.parametrize("n,npanels", [(192, 1), (320, 5), (640, 2)])
def test_dump_outputs_of_column_panels(tmp_path, n, npanels):
    """The dump of a product held as column panels (one panel on one GPU, Q x P sub-panels on rank 0 of a grid) on host tensors:
    sampled rows bit for bit, parities of every row and column, odd row and word counts included."""
    import torch
    import bench
    words = g.random_words(n, n, 7)
    full = torch.from_numpy(words.view(np.int64).copy())
    pw = (n // 64) // npanels
    panels = [full[:, i * pw:(i + 1) * pw].contiguous() for i in range(npanels)]
    shapes = bench._dump_outputs(str(tmp_path), panels, n, budget_bytes=4 * n * 7)
    assert shapes == {"C_sample_rows": [7, n], "C_sample_row_index": [7], "C_row_parity": [n], "C_col_parity": [n]}
    _check_dump(_load(str(tmp_path)), g.words_to_bits(words, n), 7)


def _run_bench(args, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_and_its_dump(built, tmp_path):
    """A plain one-GPU run: the line carries the headline fields for exactly --steps timed steps and none of the --full legs; the
    dump is the oracle's product of the seeded operands (A seed 1, B seed 2) and the same in a second run."""
    n = 4096
    outs = []
    for run in ("a", "b"):
        out = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dim", str(n), "--dump-outputs", run], tmp_path)
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["dtype"] == "u64"
        assert out["metric"] == "gf2_matmul_bit_ops_per_sec_n%d" % n and out["unit"] == "bit-ops/s" and out["higher_is_better"] is True
        assert abs(out["value"] - 2.0 * n ** 3 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
        for leg in ("cpu_baseline", "parity_sha256_ok", "configs", "elimination", "host_path"):
            assert leg not in out, leg
        outs.append(_load(str(tmp_path / run)))
    ref = g.o_mul_fast(g.random_words(n, n, 1), g.random_words(n, n, 2), n, n, n)
    _check_dump(outs[0], g.words_to_bits(ref, n), (32 << 20) // (4 * n))
    for k in DUMPED:
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.gpu
def test_bench_dump_of_a_two_rank_grid(built, tmp_path):
    """--dump-outputs on rank 0 of a 1 x 2 grid (two ranks over gloo sharing the GPU, 2 x 2 sub-panels of C gathered there)."""
    n = 4096
    out = _run_bench(["--gpus", "2", "--backend", "gloo", "--grid", "1x2", "--bcast", "broadcast", "--dim", str(n), "--no-cpu",
                      "--steps", "2", "--warmup", "1", "--dump-outputs", "d"], tmp_path)
    assert out["n_gpus"] == 2 and out["config"]["grid"] == "1x2" and out["steps"] == 2
    ref = g.o_mul_fast(g.random_words(n, n, 1), g.random_words(n, n, 2), n, n, n)
    _check_dump(_load(str(tmp_path / "d")), g.words_to_bits(ref, n), (32 << 20) // (4 * n))

"""A plain ``bench.py --gpus 1 --steps K --warmup W`` run and ``--dump-outputs``.

The plain run is the headline measurement alone: its line carries ``value``, ``ms_per_step``
and the roofline of the timed steps, and none of the blocks ``--full`` measures with launches
of their own.  ``--dump-outputs DIR`` writes what the last timed step computed; here that is
compared with the C oracle on the dump's seeded sample of a batch larger than the sample
(odd size, no multiple of the kernel's tile), and on the counts of every tuple.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path, oracle_lib, example_key):
    import bench
    n, steps, H, Q = bench.DUMP_SAMPLE + 1_000_001, 3, 128, 24
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "1", "--tuples-per-gpu", str(n), "--placement-probe", "2",
           "--placement-rounds", "1", "--settle-ms", "50", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == bench.METRIC and rec["unit"] == "tuples/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u32" and rec["full"] is False
    assert rec["steps"] == steps and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["ms_per_step"] > 0
    assert abs(rec["value"] - n / (rec["ms_per_step"] / 1e3)) < 1e-6 * rec["value"]
    assert 0 < rec["roofline"]["kernel_ms"] <= rec["ms_per_step"] * 1.001
    assert rec["placement"]["candidates"] == {"inputs": 2, "outputs": 2}
    for moved in ("counts_only", "queue_u32", "flow_like", "configs3", "configs4",
                  "row_f_kernels", "bucketed"):
        assert moved not in rec, moved
    assert rec["cpu_baseline"] is None and rec["verified"] is None
    assert "kernel_ms_min_max" not in rec["roofline"]

    got = {name: np.load(out_dir / name) for name in os.listdir(out_dir)}
    assert sorted(got) == ["counts.npy", "hash_result.npy", "queue_number.npy"]
    tup = oracle_lib.generate(bench.SEED, 0, n)
    h, q, c = oracle_lib.run(example_key, tup, H, Q, fn="oracle_run_tables")
    idx = np.sort(np.random.default_rng(bench.SEED).integers(0, n, bench.DUMP_SAMPLE))
    np.testing.assert_array_equal(got["counts.npy"], c.astype(np.float64))
    np.testing.assert_array_equal(got["hash_result.npy"], h[idx].astype(np.float64))
    np.testing.assert_array_equal(got["queue_number.npy"], q[idx].astype(np.float32))

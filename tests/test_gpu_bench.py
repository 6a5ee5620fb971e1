"""bench.py's plain run: exactly --steps timed steps in one region, the headline line only, and --dump-outputs (the same arguments give the same
inputs, so two runs dump the same outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_times_exactly_the_steps_and_dumps_the_last_one(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dumps = [tmp_path / "a", tmp_path / "b"]
    for d in dumps:
        line = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert line["steps"] == 3 and line["warmup"] == 1 and line["timed_regions"] == 1 and line["unit"] == "frames/s" and line["dtype"] == "f32"
        n_seq = line["config"]["sequences_per_gpu"]
        assert line["ms_per_step"] > 0 and abs(line["value"] - n_seq * 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["details_file"] is None and "exact_fp32_value" not in line
    names = sorted(os.listdir(dumps[0]))
    assert names == sorted(os.listdir(dumps[1]))
    n_seq = line["config"]["sequences_per_gpu"]
    assert len(names) == n_seq * 16 and all(f"seq{s}_features.npy" in names and f"seq{s}_IA11.npy" in names for s in range(n_seq))
    assert sum(os.path.getsize(dumps[0] / n) for n in names) <= 64 * 10 ** 6
    for n in names:
        a, b = np.load(dumps[0] / n), np.load(dumps[1] / n)
        assert a.dtype == np.float32 and a.shape == b.shape and a.size > 0, n
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=n)

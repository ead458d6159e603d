"""bench.py's plain line and --dump-outputs on the GPU: the headline alone, and what the last timed step computed written as
float .npy files, the same from run to run (seeded inputs)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    got = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(str(d), "*.npy"))}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    return got


def test_plain_line_is_the_headline_and_its_outputs_repeat(tmp_path):
    base = ["--gpus", "1", "--n", "2500", "--d", "64", "--steps", "3", "--warmup", "1"]
    runs = []
    for k in range(2):
        line = _bench(base + ["--dump-outputs", str(tmp_path / ("run%d" % k))])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert not {"roofline", "phases_ms", "cpu_baseline", "other_workloads"} & set(line)
        got = _load(tmp_path / ("run%d" % k))
        assert sorted(got) == ["info", "logdet", "logpdf", "quad"]
        assert got["logpdf"][0] == line["result"]["logpdf"] and got["logdet"][0] == line["result"]["logdet"]
        assert got["info"][0] == 0 and np.isfinite(got["quad"][0])
        runs.append(got)
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name


def test_conv_config_dumps_a_row_sample_of_its_kernel_matrix(tmp_path):
    line = _bench(["--config", "c3", "--n", "300", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert line["cpu_baseline"] is None
    got = _load(tmp_path)
    assert sorted(got) == ["info", "kernel_row_index", "kernel_rows", "logdet", "logpdf", "quad"]
    rows, idx = got["kernel_rows"], got["kernel_row_index"].astype(int)
    assert rows.shape == (64, 300) and len(idx) == 64 and np.all(np.diff(idx) > 0)
    lower = np.arange(300)[None, :] <= idx[:, None]
    assert np.isfinite(rows[lower]).all() and np.all(rows[~lower] == 0)
    assert np.all(rows[np.arange(64), idx] > 0)                        # the kernel's diagonal
    assert got["logpdf"][0] == line["result"]["logpdf"]

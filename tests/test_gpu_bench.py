"""bench.py on one GPU, on a small tree: a plain run prints the headline line and nothing that --full adds; --full adds the parity
check, the CPU baseline and the roofline; --dump-outputs writes the same files for the same arguments, in the table's precision,
at most 64 MB in all, each a clique belief that sums to the Z of the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--cliques", "15", "--width", "12", "--sep", "6"]


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = [ln for ln in res.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout.decode()
    return json.loads(lines[0])


def test_plain_line_and_full_line():
    plain = run_bench()
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["unit"] == "GB/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32" and plain["metric"]
    assert not {"roofline", "cpu_baseline", "parity", "configs"} & set(plain)
    full = run_bench("--full")
    assert full["config"]["Z"] == plain["config"]["Z"]
    assert full["parity"]["rel_err"] < 1e-6 and full["cpu_baseline"]["value"] > 0
    assert full["roofline"]["bound"] == "hbm" and full["roofline"]["achieved"] > 0


def test_dump_outputs_are_the_same_for_the_same_arguments(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    z = run_bench("--dump-outputs", str(a))["config"]["Z"]
    run_bench("--dump-outputs", str(b))
    names = sorted(os.listdir(a))
    assert len(names) == 15 and names == sorted(os.listdir(b))        # (15 beliefs of 16 KiB: the whole tree fits the sample)
    total = 0
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype == np.float32 and x.shape == (2,) * 12
        assert np.array_equal(x, y)
        assert abs(float(x.sum(dtype=np.float64)) - z) <= 1e-5 * abs(z)
        total += os.path.getsize(a / name)
    assert total <= 64e6

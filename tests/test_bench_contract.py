"""bench.py prints ONE JSON line with the driver's contract keys (run at the small workload so that it takes seconds): a plain run carries the
headline, --full adds the roofline, the kernel table and the CPU baseline; --dump-outputs writes what the timed path returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "roofline_hbm_kernel", "inner_loop", "kernels", "instrumented_pass", "one_at_a_time", "parity", "cpu_baseline")


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--workload", "dtu_640x480_v2_it4", *extra],
                         capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One --full run and one plain run of the same workload, each dumping its outputs."""
    base = tmp_path_factory.mktemp("bench")
    full = _bench("--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--full", "--dump-outputs", str(base / "full"))
    plain = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(base / "plain"))
    return {"full": (full, base / "full"), "plain": (plain, base / "plain")}


def test_bench_json_contract(runs):
    d, _ = runs["full"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["data"] == "synthetic"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6
    assert d["config"]["workload"] == "dtu_640x480_v2_it4" and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9


def test_plain_bench_line_is_the_headline_and_dumps_the_output(runs):
    d, dump = runs["plain"]
    full, full_dump = runs["full"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "data", "config",
              "gru_precision"):
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, f"{k}: measured by a plain run (belongs behind --full)"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6
    for k in ("metric", "unit", "dtype"):
        assert d[k] == full[k], k
    assert d["gru_precision"]["timed"] == full["gru_precision"]["timed"]
    disp = np.load(dump / "disparity.npy")
    assert disp.dtype == np.float32 and disp.shape == (1, 1, 480 // 4, 640 // 4) and np.isfinite(disp).all()
    assert np.array_equal(disp, np.load(full_dump / "disparity.npy"))        # same inputs, same arithmetic: the same depth map

"""bench.py's plain run and --dump-outputs.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) times K iterations and prints the
result line without the figures that take runs of their own (roofline, ttfs,
cpu_baseline: --full).  --dump-outputs DIR writes the tree those iterations left; here it
is compared bit for bit with a planner driven through the same calls, and the sampling of
a tree above DUMP_MAX_ROWS rows is checked on a stand-in planner (CPU).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits

BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("tree_samples", "tree_parents", "tree_costs", "tree_rows", "iter_log")


class _Planner:
    """iter_log() and tree() of a planner whose tree holds `rows` rows."""

    def __init__(self, rows, capacity):
        rng = np.random.default_rng(7)
        self.s = rng.standard_normal((capacity, 7)).astype(np.float32)
        self.p = rng.integers(-1, rows, capacity).astype(np.int32)
        self.c = rng.random(capacity).astype(np.float32)
        self.log = np.zeros((3, 9), dtype=np.int64)
        self.log[:, 7] = (rows - 2, rows - 1, rows)

    def iter_log(self):
        return self.log

    def tree(self):
        return self.s, self.p, self.c


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_writes_every_row_of_a_small_tree(tmp_path):
    import bench
    pl = _Planner(rows=1000, capacity=1500)
    bench.dump_outputs(pl, str(tmp_path / "d"))
    a = _load(tmp_path / "d")
    assert a["tree_samples"].dtype == np.float32 and a["tree_costs"].dtype == np.float32
    assert a["tree_parents"].dtype == a["tree_rows"].dtype == a["iter_log"].dtype == np.float64
    assert np.array_equal(a["tree_rows"], np.arange(1000))
    assert np.array_equal(bits(a["tree_samples"]), bits(pl.s[:1000]))
    assert np.array_equal(a["tree_parents"], pl.p[:1000]) and np.array_equal(bits(a["tree_costs"]), bits(pl.c[:1000]))
    assert np.array_equal(a["iter_log"], pl.log)


def test_dump_samples_a_large_tree_the_same_way_every_time(tmp_path):
    import bench
    rows = bench.DUMP_MAX_ROWS + 12345
    pl = _Planner(rows=rows, capacity=rows + 10)
    bench.dump_outputs(pl, str(tmp_path / "a"))
    bench.dump_outputs(pl, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    keep = a["tree_rows"].astype(np.int64)
    assert len(keep) == bench.DUMP_MAX_ROWS and (np.diff(keep) > 0).all() and 0 <= keep[0] and keep[-1] < rows
    assert np.array_equal(bits(a["tree_samples"]), bits(pl.s[keep])) and np.array_equal(a["tree_parents"], pl.p[keep])
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for n in NAMES:
        assert a[n].tobytes() == b[n].tobytes(), n


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_tree_of_its_last_step(tmp_path):
    import bench
    from cudasbmp_amd import KGMT, DeviceBuffer, read_obstacles_csv
    from cudasbmp_amd.config import workload
    W, K = 2, 3
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == K and out["warmup"] == W and out["unit"] == "samples/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"roofline", "ttfs", "cpu_baseline"} & set(out), "figures of --full in a plain run"
    a = _load(tmp_path / "d")
    log = a["iter_log"]
    assert len(log) == W + K   # --steps sets the number of timed iterations
    # value = the timed iterations' children over K x ms_per_step (rounded to 0.1 us in the line)
    assert out["value"] == pytest.approx(log[W:, 5].sum() / (K * out["ms_per_step"] * 1e-3), rel=0.02)

    cfg = workload("c3")   # the same planner calls, here
    obs = read_obstacles_csv(cfg["obstacles"])
    pl = dict(cfg["planner"], numIterations=W + K + 2)
    g = KGMT(**pl, samplesPerIteration=cfg["samplesPerIteration"], agent=cfg["agent"], batchRule=cfg["batchRule"],
             fixGNewClear=True)
    g.begin(cfg["initial"], cfg["goal"], DeviceBuffer(obs), len(obs), bench.SEED)
    g.enqueue(W + K)
    g.fold()
    g.sync()
    assert np.array_equal(log, g.iter_log())
    rows = int(log[-1, 7])
    s, p, c = g.tree()
    assert rows > 0 and np.array_equal(a["tree_rows"], np.arange(rows))
    assert np.array_equal(bits(a["tree_samples"]), bits(s[:rows]))
    assert np.array_equal(a["tree_parents"], p[:rows]) and np.array_equal(bits(a["tree_costs"]), bits(c[:rows]))

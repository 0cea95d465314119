"""Every scenario of tests/scenarios.py through the CPU oracle alone: the scenario must
reach the edge it is aimed at (its `cover` conditions), so that one which stops doing so
fails here, without a GPU, instead of silently testing nothing on the GPU.

The conditions are properties of the oracle's run, not measurements of the kernels.
"""
import functools
import hashlib

import numpy as np
import pytest

from scenarios import IDS, SCENARIOS, make_oracle

LOG = {n: i for i, n in enumerate(("itr", "treeSizeBefore", "nG", "k", "nExp", "S", "A", "treeSizeAfter", "goalIdx"))}
ONE_WAVE = 64   # crossings asked for: one wave's worth of rows


def _digest(o):
    """(treeSize, hash of the tree arrays): the oracle's result for the F comparisons."""
    n = min(o.info()["treeSize"], o.M)
    s, p, c = o.tree()
    h = hashlib.sha256()
    for a in (s[:n], p[:n], c[:n]):
        h.update(np.ascontiguousarray(a).tobytes())
    return o.info()["treeSize"], h.hexdigest()


def crossings(o, limit, strict_parent):
    """Tree rows whose |theta| lies on the other side of `limit` than their parent's:
    (upwards, downwards).  Upwards is parent <= limit < own, or with strict_parent
    parent < limit <= own (car_theta_bounded's B < 100000)."""
    n = min(o.info()["treeSize"], o.M)
    s, p, _ = o.tree()
    own = np.abs(s[1:n, 2].astype(np.float64))
    par = np.abs(s[p[1:n], 2].astype(np.float64))
    if strict_parent:
        up = (par < limit) & (own >= limit)
        down = (par >= limit) & (own < limit)
    else:
        up = (par <= limit) & (own > limit)
        down = (par > limit) & (own <= limit)
    return int(up.sum()), int(down.sum())


def schedule_shape(log):
    """(iterations with 64 <= k < 256 and |G| >= 64, iterations with 1 < k < 32)."""
    k, nG = log[:, LOG["k"]], log[:, LOG["nG"]]
    return int(((k >= 64) & (k < 256) & (nG >= 64)).sum()), int(((k > 1) & (k < 32)).sum())


@functools.lru_cache(maxsize=None)
def _digest_without(name):
    sc = next(s for s in SCENARIOS if s.name == name)
    return _digest(make_oracle(sc, obstacles=np.delete(sc.obstacles(), list(sc.added_rows), axis=0)))


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_scenario_reaches_its_edge(sc, oracle_lib):
    o = make_oracle(sc)
    log = o.iter_logs()
    info = o.info()
    reg = o.regions()
    cfg, _ = sc.config()
    W, H = np.float32(cfg["width"]), np.float32(cfg["height"])
    n = min(info["treeSize"], o.M)
    s, p, _ = o.tree()
    assert "spread" in sc.cover or "stall" in sc.cover
    for cond in sc.cover:
        kind, arg = (cond, None) if isinstance(cond, str) else cond
        if kind == "spread":
            expanding = int((log[:, LOG["S"]] > 0).sum())
            valid, invalid = int(reg["R1Valid"].sum()), int(reg["R1Invalid"].sum())
            assert expanding >= 3, f"{expanding} expanding iterations"
            assert min(valid, invalid) >= 0.05 * (valid + invalid), f"valid {valid}, invalid {invalid}"
        elif kind == "stall":
            assert info["treeSize"] == 1
        elif kind == "schedule":
            wide, narrow = schedule_shape(log)
            assert wide >= 2 and narrow >= 2, f"k = {log[:, LOG['k']].tolist()}, |G| = {log[:, LOG['nG']].tolist()}"
        elif kind == "cross_both":
            up, down = crossings(o, arg, strict_parent=False)
            assert up >= ONE_WAVE and down >= ONE_WAVE, f"{up} rows cross {arg} upwards, {down} downwards"
        elif kind == "cross_up":
            up, _ = crossings(o, arg, strict_parent=True)
            assert up >= ONE_WAVE, f"{up} rows cross {arg} upwards"
        elif kind == "tree_x_beyond":
            assert (s[:n, 0] > np.float32(arg)).any()
        elif kind == "uncounted_y_beyond":
            # R1Size = width / N on both axes (the reference's): a child with W <= y < H is
            # inside the workspace and outside the R1 grid, so no table counts it (D3)
            stepped, beyond = make_oracle(sc, plan=False), 0
            while stepped.step():
                u, _ = stepped.unexplored()   # the last child each slot held
                beyond += int(((u[:, 1] >= W) & (u[:, 1] < H) & (u[:, 0] > 0) & (u[:, 0] < W)).sum())
            assert beyond > 0
            assert int(reg["R1"].sum()) < info["samples"]
            assert not (s[1:n, 1] >= W).any(), "a child outside the R1 grid was inserted"
        elif kind == "box_changes":
            assert _digest(o) != _digest_without(sc.name)
        elif kind == "box_neutral":
            assert _digest(o) == _digest_without(sc.name)
        else:
            raise AssertionError(f"unknown coverage condition {cond!r}")

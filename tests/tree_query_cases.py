"""Crafted rows and goals for the goal query (include/sbmp/tree_query.h), shared by the CPU
tests of the host twin (tests/test_tree_query.py) and the GPU tests of k_tree_query
(tests/test_gpu_tree_query.py).  Plain numpy: no GPU and no library at import.

A case is (state (R, 4), ctrl (R, 4), goals (Q, 3), expect): the planner's tree layout, state
= (x, y, -, -) and ctrl = (-, -, -, cost), and expect = [(goal, field, value), ...], what the
case was built to show.  Every answer is also compared with the numpy model as a whole; the
model of a case is computed once (case()) and only read afterwards.

The background rows lie on a lattice near (1000, 2000), far from every goal, so that a goal's
inside rows are exactly the rows a case plants.  k_tree_query takes 2,048 rows per workgroup
and step (256 lanes x 8 rows) on a grid of at most 8 workgroups per CU, so one sweep of the
grid is at most 256 x 8 x 2,048 = 4,194,304 rows on an MI355X; BIG is 77 rows more.
"""
from __future__ import annotations

import functools

import numpy as np

from tree_query_model import d2_of, model_of_rows

BIG = (1 << 22) + 77
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, BIG)
GOAL_COUNTS = (1, 7, 8, 9, 63, 64, 65, 257)
DENORM_MIN = np.float32(1e-45)   # the smallest subnormal


def background(R: int):
    i = np.arange(R, dtype=np.int64)
    state = np.zeros((R, 4), np.float32)
    state[:, 0] = (1000.0 + (i % 4093) * 0.125).astype(np.float32)
    state[:, 1] = (2000.0 + (i // 4093) * 0.125).astype(np.float32)
    state[:, 2] = 0.5
    ctrl = np.zeros((R, 4), np.float32)
    ctrl[:, 2] = 0.25
    ctrl[:, 3] = (1.0 + ((i * 7) % 1021) * 0.25).astype(np.float32)
    return state, ctrl


def _plant(state, ctrl, row, x, y, cost):
    state[row, 0], state[row, 1], ctrl[row, 3] = np.float32(x), np.float32(y), np.float32(cost)


def single(R: int):
    """One inside row per goal, at rows 0, 63, 64, 255, 256 and R - 1 (those that exist)."""
    state, ctrl = background(R)
    rows = sorted({p for p in (0, 63, 64, 255, 256, R - 1) if p < R})
    goals, expect = [], []
    for k, p in enumerate(rows):
        cx, cy = 10.0 + 8.0 * k, 10.0
        _plant(state, ctrl, p, cx + 0.125, cy, 3.0 + k)
        goals.append((cx, cy, 0.5))
        expect += [(k, "count", 1), (k, "firstRow", p), (k, "bestRow", p), (k, "nearestRow", p),
                   (k, "bestCost", np.float32(3.0 + k)), (k, "nearestDistance", np.float32(0.125))]
    return state, ctrl, goals, expect


def ties():
    R = 5000   # three workgroups: rows [0, 2048), [2048, 4096), [4096, 5000)
    state, ctrl = background(R)
    # goal 0: two inside rows of equal cost, rows 5 and R - 1
    _plant(state, ctrl, 5, 10.125, 10.0, 2.5)
    _plant(state, ctrl, R - 1, 10.0, 10.25, 2.5)
    # goal 1: two rows of equal d2 (0.25^2 either side of the centre), far apart; the farther is cheaper
    _plant(state, ctrl, 7, 30.25, 10.0, 9.0)
    _plant(state, ctrl, R - 2, 29.75, 10.0, 4.0)
    # goal 2: rows 3 and 4100 (another workgroup) are equal, and both the cheapest and the nearest
    _plant(state, ctrl, 3, 50.125, 10.0, 1.5)
    _plant(state, ctrl, 4100, 50.125, 10.0, 1.5)
    _plant(state, ctrl, 2000, 50.25, 10.25, 6.0)
    # goal 3: the root (cost +0) inside
    _plant(state, ctrl, 0, 10.125, 30.0, 0.0)
    _plant(state, ctrl, 100, 10.0, 30.0625, 0.5)
    goals = [(10.0, 10.0, 0.5), (30.0, 10.0, 0.5), (50.0, 10.0, 0.5), (10.0, 30.0, 0.5)]
    expect = [(0, "count", 2), (0, "firstRow", 5), (0, "bestRow", 5),
              (1, "count", 2), (1, "nearestRow", 7), (1, "bestRow", R - 2),
              (2, "count", 3), (2, "bestRow", 3), (2, "nearestRow", 3), (2, "firstRow", 3),
              (3, "count", 2), (3, "bestRow", 0), (3, "firstRow", 0), (3, "bestCost", np.float32(0.0)),
              (3, "nearestRow", 100)]
    return state, ctrl, goals, expect


def radius_edges():
    """Row k at distance d: r = d leaves it outside (strict), the next float up takes it in, the
    next float down leaves it outside; the two nearer rows stay inside, the farther one outside."""
    R, k = 300, 137
    state, ctrl = background(R)
    _plant(state, ctrl, 20, 10.1, 10.1, 2.0)
    _plant(state, ctrl, 250, 9.9, 10.15, 3.0)
    _plant(state, ctrl, k, 10.3, 10.4, 1.25)
    _plant(state, ctrl, 290, 10.6, 10.7, 1.0)
    d2 = d2_of(state[k:k + 1, 0], state[k:k + 1, 1], 10.0, 10.0)
    d = np.sqrt(d2, dtype=np.float32)[0]
    up, down = np.nextafter(d, np.float32(np.inf)), np.nextafter(d, np.float32(0.0))
    goals = [(10.0, 10.0, d), (10.0, 10.0, up), (10.0, 10.0, down)]
    expect = [(0, "count", 2), (0, "bestRow", 20), (1, "count", 3), (1, "bestRow", k), (2, "count", 2),
              (2, "bestRow", 20), (0, "firstRow", 20), (1, "firstRow", 20), (2, "firstRow", 20)]
    return state, ctrl, goals, expect


def zero_distance():
    R = 257
    state, ctrl = background(R)
    _plant(state, ctrl, 200, 12.5, 7.25, 4.0)
    goals = [(12.5, 7.25, DENORM_MIN)]
    expect = [(0, "count", 1), (0, "firstRow", 200), (0, "bestRow", 200), (0, "nearestRow", 200),
              (0, "nearestDistance", np.float32(0.0))]
    return state, ctrl, goals, expect


def degenerate():
    R = 2500
    state, ctrl = background(R)
    ctrl[0, 3] = 0.0   # the root: the cheapest row
    _plant(state, ctrl, 1234, 10.0, 10.0, 2.0)   # on the centre: d2 = 0 is still not inside r <= 0
    radii = [0.0, -0.0, -1.0, -np.inf, np.nan, np.inf]
    goals = [(10.0, 10.0, r) for r in radii]
    expect = []
    for q in range(5):
        expect += [(q, "count", 0), (q, "firstRow", -1), (q, "bestRow", -1), (q, "bestCost", np.float32(0.0)),
                   (q, "nearestRow", 1234), (q, "nearestDistance", np.float32(0.0))]
    expect += [(5, "count", R), (5, "firstRow", 0), (5, "bestRow", 0), (5, "nearestRow", 1234)]
    return state, ctrl, goals, expect


def goal_count(Q: int):
    """Q goals over 3,000 scattered rows: either side of every power-of-two tile up to 256."""
    R = 3000
    rng = np.random.default_rng(100 + Q)
    state = np.zeros((R, 4), np.float32)
    state[:, :2] = rng.uniform(0.0, 20.0, size=(R, 2)).astype(np.float32)
    ctrl = np.zeros((R, 4), np.float32)
    ctrl[:, 3] = rng.uniform(0.0, 30.0, size=R).astype(np.float32)
    goals = np.concatenate([rng.uniform(0.0, 20.0, size=(Q, 2)), rng.uniform(0.8, 1.6, size=(Q, 1))], axis=1)
    return state, ctrl, goals.astype(np.float32), []


def overflow():
    R = 300
    state, ctrl = background(R)
    goals = [(3e38, 0.0, 1.0)]   # dx * dx overflows: d2 = inf for every row
    expect = [(0, "count", 0), (0, "nearestRow", 0), (0, "nearestDistance", np.float32(np.inf))]
    return state, ctrl, goals, expect


def random_rows():
    R = 20000
    rng = np.random.default_rng(7)
    state = rng.uniform(0.0, 20.0, size=(R, 4)).astype(np.float32)
    ctrl = rng.uniform(0.0, 30.0, size=(R, 4)).astype(np.float32)
    goals = np.concatenate([rng.uniform(-1.0, 21.0, size=(40, 2)), rng.uniform(0.0, 3.0, size=(40, 1))], axis=1)
    return state, ctrl, goals.astype(np.float32), []


BUILDERS = {f"single-{R}": functools.partial(single, R) for R in ROW_COUNTS}
BUILDERS.update({"ties": ties, "radius-edges": radius_edges, "zero-distance": zero_distance,
                 "degenerate": degenerate, "overflow": overflow, "random": random_rows})
BUILDERS.update({f"goals-{Q}": functools.partial(goal_count, Q) for Q in GOAL_COUNTS})
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(state, ctrl, goals (Q, 3) float32, expect, model): built and modelled once, read-only."""
    state, ctrl, goals, expect = BUILDERS[name]()
    goals = np.asarray(goals, dtype=np.float32).reshape(-1, 3)
    model = model_of_rows(state, ctrl, goals)
    for a in (state, ctrl, goals, *model.values()):
        a.setflags(write=False)
    return state, ctrl, goals, tuple(expect), model


def check_expect(answers: dict, expect, label: str = "") -> None:
    for q, field, value in expect:
        got = answers[field][q]
        if isinstance(value, np.float32):
            assert np.float32(got).view(np.uint32) == value.view(np.uint32), f"{label} goal {q} {field}: {got} != {value}"
        else:
            assert int(got) == int(value), f"{label} goal {q} {field}: {got} != {value}"

"""The case table of the adoption tests (tests/test_tree_adopt.py, tests/test_gpu_tree_adopt.py):
crafted rows, grids, goal discs and frontiers at every seam of include/sbmp/tree_adopt.h and of
the k_adopt_* kernels.  Every base case appears twice, with a NULL goal disc and with a disc.

  rows-R          R = 1, 2, 63, 64, 65, 255, 256, 257, 1,023, 1,024, 1,025 random rows: one lane, a
                  wave and a workgroup of the scan, each one short, full and one over; several workgroups
  one-cell        65,537 rows in one R2 cell: an R1 count past 16 bits, one atomicOr target for every lane
  r1-lines        rows on every R1 line of both axes and one ulp either side
  r2-lines        likewise on R2 lines
  round-up        a width at which fl(v / R1Size) lands on a line the real quotient stays below
                  (region_scenarios.round_up_widths)
  outside         rows outside the workspace on each side, near and far
  nonfinite       NaN and +-inf rows below and inside the frontier
  goal-edge       rows at the disc's radius exactly and one ulp either side; several inside, the lowest wins
  frontier-*      frontierFrom at 0, R - 1 and R
  grid-*          N = 1, n = 1, both, the demo's grid (16, 8), the largest (16, 16), W != H
  rows-sweep+77, rows-2sweep+1   random rows past one sweep of the grid (SWEEP = 524,288 rows): the later
                  rounds of k_adopt_scan and k_adopt_seed; the disc holds rows of every sweep
  goal-past-sweep       the one row inside the disc is row SWEEP + 40
  goal-both-sweeps      inside rows at r and r + SWEEP, three r in one wave and two in other waves: the lowest wins
  counters-past-sweep   non-finite and out-of-grid rows at or past row SWEEP only, on both sides of
                  a frontier that starts at SWEEP + 10

Plain numpy; no GPU and no library at import.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import tree_adopt_model as model
from tree_query_cases import SWEEP

F32 = np.float32
ROW_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
ONE_CELL_ROWS = 65537
PAST_SWEEP = (("rows-sweep+77", SWEEP + 77), ("rows-2sweep+1", 2 * SWEEP + 1))
GOAL_BOTH = (643, 650, 700, 760, 1090)         # and the rows one sweep above them
COUNTERS_NONFINITE = (2, 5, 9, 12, 30, 64, 70)  # rows past SWEEP; the frontier starts at SWEEP + 10
COUNTERS_OUTSIDE = (3, 7, 50, 63, 76)
DEMO_GRID = dict(width=20.0, height=20.0, N=16, n=8)      # demos/main.cu
DEMO_GOAL = (2.0, 18.0, 0.5)


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    state: np.ndarray          # (R, 4) float32
    width: float
    height: float
    N: int
    n: int
    goal: Optional[tuple]      # (x, y, radius) or None
    frontier_from: int

    @property
    def rows(self) -> int:
        return len(self.state)

    @property
    def grid(self) -> dict:
        return dict(width=self.width, height=self.height, N=self.N, n=self.n)

    @functools.cached_property
    def model(self) -> dict:
        return model.tables(self.state, self.width, self.N, self.n, self.goal, self.frontier_from)


def _rows(xy, theta=0.25, v=1.0) -> np.ndarray:
    xy = np.asarray(xy, dtype=F32).reshape(-1, 2)
    st = np.zeros((len(xy), 4), dtype=F32)
    st[:, :2] = xy
    st[:, 2] = theta
    st[:, 3] = v
    return st


def random_rows(R, seed, W=20.0, H=20.0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    st = np.zeros((R, 4), dtype=F32)
    st[:, 0] = rng.uniform(0.0, W, R)
    st[:, 1] = rng.uniform(0.0, H, R)
    st[:, 2] = rng.uniform(-3.0, 3.0, R)
    st[:, 3] = rng.uniform(-2.0, 2.0, R)
    return st


def line_rows(size, count, other=3.3) -> np.ndarray:
    """Rows on the lines k * size, k = 0 .. count, and one ulp either side, on x and then on y."""
    k = np.arange(count + 1, dtype=np.float64)
    on = (k * np.float64(size)).astype(F32)
    v = np.concatenate([on, np.nextafter(on, F32(np.inf)), np.nextafter(on, F32(-np.inf))])
    o = np.full(len(v), other, dtype=F32)
    return _rows(np.concatenate([np.stack([v, o], axis=1), np.stack([o, v], axis=1)]))


def round_up_case():
    """(state, width): rows whose quotient by R1Size = width / 16 rounds up onto a line."""
    from region_scenarios import round_up_widths
    rng = np.random.default_rng(3)
    for c in (3, 5, 7, 11, 13):
        v = rng.uniform(2.0, 18.0, 4000).astype(F32)
        for W, hit in round_up_widths(v, c):
            idx = np.flatnonzero(hit)
            if len(idx):
                i = idx[0]
                w = float(W[i])
                xs = np.array([v[i], up(v[i]), down(v[i])], dtype=F32)
                o = np.full(3, 1.0, dtype=F32)
                return _rows(np.concatenate([np.stack([xs, o], axis=1), np.stack([o, xs], axis=1)])), w, c
    raise AssertionError("no round-up width found")


def outside_rows(W, H) -> np.ndarray:
    xs = [-0.5, -1.5, -1e9, float(down(0.0)), W, float(up(W)), W + 3.0, 1e30, float(down(W))]
    ys = [-0.5, -1.5, -1e9, float(down(0.0)), H, float(up(H)), H + 3.0, 1e30, float(down(H))]
    xy = [(x, 4.4) for x in xs] + [(4.4, y) for y in ys] + [(-0.5, -0.5), (W + 1, H + 1), (3.0, 3.0)]
    return _rows(xy)


def nonfinite_rows() -> np.ndarray:
    st = random_rows(40, 17)
    nan, inf = np.nan, np.inf
    bad = [(0, nan), (1, inf), (2, -inf), (3, nan)]
    for base in (4, 24):                       # below and inside a frontier that starts at row 20
        for j, (col, val) in enumerate(bad * 2):
            st[base + j, col] = val
    st[14, :] = nan
    st[34, :2] = (inf, -inf)
    return st


def goal_edge_rows(goal):
    gx, gy, r = (F32(v) for v in goal)
    xs = [gx + r, up(gx + r), down(gx + r), gx - r, up(gx - r), down(gx - r)]
    xy = [(9.0, 9.0), (12.0, 3.0)] + [(x, gy) for x in xs] + [(gx, gy + r), (gx, down(gy + r))]
    xy += [(gx, gy), (gx + F32(0.1), gy), (8.0, 8.0)]
    return _rows(xy)


def _outside_the_disc(st, goal, but=()) -> np.ndarray:
    """`st` with every row inside the disc moved to (1.5, 1.5), except the rows `but`."""
    inside = model.in_goal(st[:, 0], st[:, 1], goal)
    inside[list(but)] = False
    st[inside, :2] = (1.5, 1.5)
    return st


def goal_past_sweep():
    """(state, goal): SWEEP + 77 random rows, of which row SWEEP + 40 alone lies inside the disc."""
    R, row = SWEEP + 77, SWEEP + 40
    st = random_rows(R, 41)
    st[row, :2] = (12.25, 7.5)
    goal = (12.0, 7.5, 0.5)
    st = _outside_the_disc(st, goal, but=(row,))
    assert np.flatnonzero(model.in_goal(st[:, 0], st[:, 1], goal)).tolist() == [row]
    return st, goal


def goal_both_sweeps():
    """(state, goal): the rows GOAL_BOTH and the rows one sweep above them inside the disc, no other:
    three of them in one wave (640 .. 703), one in the next wave, one in another workgroup."""
    R = SWEEP + 1100
    goal = (12.0, 7.5, 0.5)
    st = _outside_the_disc(random_rows(R, 43), goal)
    rows = np.array(GOAL_BOTH + tuple(r + SWEEP for r in GOAL_BOTH))
    st[rows, 0] = np.linspace(11.8, 12.2, len(rows), dtype=F32)
    st[rows, 1] = 7.5
    assert np.array_equal(np.flatnonzero(model.in_goal(st[:, 0], st[:, 1], goal)), np.sort(rows))
    return st, goal


def counters_past_sweep() -> np.ndarray:
    """SWEEP + 77 rows whose non-finite and out-of-grid rows all lie at or past row SWEEP; the
    frontier starts at SWEEP + 10, so rows COUNTERS_NONFINITE lie on both sides of it."""
    st = random_rows(SWEEP + 77, 47)
    for i, r in enumerate(COUNTERS_NONFINITE):
        st[SWEEP + r, i % 4] = (np.nan, np.inf, -np.inf, np.nan)[i % 4]
    for i, r in enumerate(COUNTERS_OUTSIDE):
        st[SWEEP + r, i % 2] = (-1.0, 25.0, 20.0)[i % 3]
    return st


@functools.lru_cache(maxsize=None)
def planner_past_sweep():
    """(state, ctrl, parent, frontier_from) of the planner-level adoption past one sweep: SWEEP + 77
    random rows inside the workspace, random lower parents, distinct costs, the frontier at the last
    64 rows.  k_adopt_seed copies them into the planner's tree, which only the planner entry asks for."""
    R = SWEEP + 77
    rng = np.random.default_rng(51)
    state = random_rows(R, 51)
    ctrl = np.zeros((R, 4), dtype=F32)
    ctrl[:, 0] = rng.uniform(-5.0, 5.0, R)
    ctrl[:, 1] = rng.uniform(-3.1, 3.1, R)
    ctrl[:, 2] = rng.uniform(0.06, 0.3, R)
    ctrl[:, 3] = rng.permutation(R).astype(F32)             # distinct: R < 2^24
    parent = (rng.random(R) * np.arange(R)).astype(np.int32)
    parent[0] = -1
    assert len(np.unique(ctrl[:, 3])) == R and (parent[1:] < np.arange(1, R)).all() and (parent[1:] >= 0).all()
    for a in (state, ctrl, parent):
        a.setflags(write=False)
    return state, ctrl, parent, R - 64


def _base_cases() -> list:
    """(name, state, grid, goal-with-disc, frontier_from)."""
    B = []
    demo = DEMO_GRID
    for R in ROW_COUNTS:
        st = random_rows(R, 100 + R)
        B.append((f"rows-{R}", st, demo, (float(st[R // 2, 0]), float(st[R // 2, 1]), 1.5), 0))
    one = np.tile(np.array([[5.01, 5.02, 0.3, 1.0]], dtype=F32), (ONE_CELL_ROWS, 1))
    B.append(("one-cell", one, demo, (5.0, 5.0, 0.5), 0))
    B.append(("r1-lines", line_rows(model.sizes(20.0, 16, 8)[0], 16), demo, DEMO_GOAL, 0))
    B.append(("r2-lines", line_rows(model.sizes(20.0, 16, 8)[1], 128), demo, DEMO_GOAL, 0))
    B.append(("r2-lines-17.3", line_rows(model.sizes(17.3, 16, 3)[1], 48), dict(width=17.3, height=20.0, N=16, n=3),
              DEMO_GOAL, 0))
    st, w, _ = round_up_case()
    B.append(("round-up", st, dict(width=w, height=20.0, N=16, n=8), DEMO_GOAL, 0))
    B.append(("outside", outside_rows(20.0, 20.0), demo, DEMO_GOAL, 0))
    B.append(("outside-12x30", outside_rows(12.0, 30.0), dict(width=12.0, height=30.0, N=16, n=8), (10.0, 27.0, 0.5), 0))
    B.append(("nonfinite", nonfinite_rows(), demo, DEMO_GOAL, 20))
    B.append(("goal-edge", goal_edge_rows(DEMO_GOAL), demo, DEMO_GOAL, 0))
    B.append(("goal-edge-up", goal_edge_rows(DEMO_GOAL), demo, DEMO_GOAL[:2] + (float(up(0.5)),), 0))
    B.append(("goal-edge-down", goal_edge_rows(DEMO_GOAL), demo, DEMO_GOAL[:2] + (float(down(0.5)),), 0))
    B.append(("goal-radius-zero", goal_edge_rows(DEMO_GOAL), demo, DEMO_GOAL[:2] + (0.0,), 0))
    st = random_rows(300, 23)
    for name, f in (("frontier-0", 0), ("frontier-last", 299), ("frontier-R", 300)):
        B.append((name, st, demo, (float(st[200, 0]), float(st[200, 1]), 2.0), f))
    st = random_rows(700, 29, 30.0, 12.0)
    st[::7, 0] = -1.0
    for name, g in (("grid-N1-n1", dict(N=1, n=1)), ("grid-N1-n16", dict(N=1, n=16)), ("grid-N16-n1", dict(N=16, n=1)),
                    ("grid-N3-n5", dict(N=3, n=5)), ("grid-largest", dict(N=16, n=16)), ("grid-demo", dict(N=16, n=8))):
        B.append((name, st, dict(width=30.0, height=12.0, **g), (27.0, 10.0, 1.0), 0))
    B.append(("grid-12x30", random_rows(700, 31, 12.0, 30.0), dict(width=12.0, height=30.0, N=16, n=8),
              (10.0, 27.0, 1.0), 350))
    for name, R in PAST_SWEEP:                 # the disc round the last row holds rows of every sweep: the lowest wins
        st = random_rows(R, 100 + R % 1000)
        B.append((name, st, demo, (float(st[R - 1, 0]), float(st[R - 1, 1]), 1.5), 0))
    st, goal = goal_past_sweep()
    B.append(("goal-past-sweep", st, demo, goal, 0))
    st, goal = goal_both_sweeps()
    B.append(("goal-both-sweeps", st, demo, goal, 0))
    B.append(("counters-past-sweep", counters_past_sweep(), demo, (10.0, 10.0, 1.0), SWEEP + 10))
    return B


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}
    for name, st, grid, goal, f in _base_cases():
        st = np.ascontiguousarray(st, dtype=F32)
        st.setflags(write=False)
        out[name + "-nogoal"] = Case(name + "-nogoal", st, grid["width"], grid["height"], grid["N"], grid["n"], None, f)
        out[name + "-disc"] = Case(name + "-disc", st, grid["width"], grid["height"], grid["N"], grid["n"],
                                   tuple(float(v) for v in goal), f)
    return out


def _ids() -> tuple:
    names = [f"rows-{R}" for R in ROW_COUNTS] + [
        "one-cell", "r1-lines", "r2-lines", "r2-lines-17.3", "round-up", "outside", "outside-12x30", "nonfinite",
        "goal-edge", "goal-edge-up", "goal-edge-down", "goal-radius-zero", "frontier-0", "frontier-last", "frontier-R",
        "grid-N1-n1", "grid-N1-n16", "grid-N16-n1", "grid-N3-n5", "grid-largest", "grid-demo", "grid-12x30"]
    names += [name for name, _ in PAST_SWEEP] + ["goal-past-sweep", "goal-both-sweeps", "counters-past-sweep"]
    return tuple(n + s for n in names for s in ("-nogoal", "-disc"))


CASE_IDS = _ids()          # the names of cases(), known without building the rows


def case(cid) -> Case:
    return cases()[cid]

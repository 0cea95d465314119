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

Plain numpy; no GPU and no library at import.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import tree_adopt_model as model

F32 = np.float32
ROW_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
ONE_CELL_ROWS = 65537
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
    return tuple(n + s for n in names for s in ("-nogoal", "-disc"))


CASE_IDS = _ids()          # the names of cases(), known without building the rows


def case(cid) -> Case:
    return cases()[cid]

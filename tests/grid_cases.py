"""Segments and box lists that hold the device forms of the uniform-grid obstacle index
(grid_run / grid_run_sep / grid_free_at and grid_motion_valid_batched) to brute force where a
planner run of slow children never takes them: spans of three and more cell rows, runs longer
than one, two and four batches, the run that ends the box array, G = 1 and G = 90, segments
that start outside the workspace, W != H.

Three parts, none of which reads the library:

  the index     a numpy restatement of include/sbmp/obstacle_grid.h's layout: cell() in float32,
                the planner's resolution min(grid_resolution(n), 90), the CSR start table and the
                per-cell box order (ascending box index), and walk(), the query over it, with
                switches for the wrong walks a case must catch:
                  a  stops after the first two cell rows
                  b  stops after the first batch (B boxes) of a run
                  c  column range one short (cx1 exclusive)
                  d  row range one short (cy1 exclusive)
                  e  no clamp of the cell index: cy * G + cx with the raw floor; a table address
                     outside [0, G * G] reads an empty run
                  f0 .. f3  `<` for `<=` in maxx <= o.x, o.z <= minx, maxy <= o.y, o.w <= miny
                  g  ignores the last box of a run
  polylines     Cases of tests/tree_recheck_cases.py for the point agent with numDisc = 1: row r
                is the child of row r - 1 with controls (vx, vy, 1, 0) and stored state
                (fl(x + vx), fl(y + vy), 0, 0), so sbmp_tree_recheck_batch replays the segment
                row r - 1 -> row r through point_euler in whatever obstacle form is selected.
                Poly builds them: every hop is asserted exact in float32 (x + fl(x' - x) == x'),
                and goto() inserts rows over 1/64-lattice points where one hop would round.
  scenarios     planner Scenarios whose children make long segments over dense lists, for
                k_step's B = 8 LDS-table form, with steps(): every slot's segment of every
                iteration, from the stepped CPU oracle.

tests/test_grid_cases_oracle.py proves the coverage on the CPU; tests/test_gpu_grid_cases.py
runs the same cases on the kernels.  Plain numpy plus the CPU oracle at call time; no GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from scenarios import Scenario, make_oracle, random_boxes
from tree_recheck_cases import Case
from tree_recheck_model import BLOCKED, CUT, FREE

F = np.float32
MAX_G = 90                      # kMaxLdsGridG: the planner's and the re-check's cap on G
B_GLOBAL, B_LDS = 4, 8          # boxes per batch: the global table (k_expand, k_tree_recheck), k_step's LDS table
SWITCHES = ("a", "b", "c", "d", "e", "f0", "f1", "f2", "f3", "g")
NAN = float("nan")
INF = float("inf")


def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


# ---------------------------------------------------------------- the index
def cell(v, inv, g, clamp=True):
    """clamp(floor(v * inv), 0, g - 1) with the product in float32; NaN maps to 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(v, F) * F(inv))
    assert f.dtype == F
    if not clamp:
        return f.astype(np.int64)
    f = np.where(f >= 0, f, F(0))                 # false for NaN
    return np.minimum(f, F(g - 1)).astype(np.int64)


def resolution(n):
    g = 1
    while g < 256 and 2 * g * g < n:
        g += 1
    return g


def planner_g(n):
    return min(resolution(n), MAX_G)


@dataclass(frozen=True, eq=False)
class Index:
    g: int
    invW: np.float32
    invH: np.float32
    start: np.ndarray            # (g * g + 1,) CSR offsets, row-major cells
    order: np.ndarray            # (start[-1],) box index of every entry
    rows: np.ndarray             # (start[-1], 4) the boxes in entry order


def build_index(boxes, W, H, g=None) -> Index:
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    n = len(boxes)
    g = planner_g(n) if g is None else g
    invW, invH = F(g) / F(W), F(g) / F(H)
    nan = np.isnan(boxes).any(axis=1)
    a, c = cell(boxes[:, 0], invW, g), cell(boxes[:, 2], invW, g)
    e, f = cell(boxes[:, 1], invH, g), cell(boxes[:, 3], invH, g)
    x0, x1 = np.where(nan, 0, np.minimum(a, c)), np.where(nan, g - 1, np.maximum(a, c))
    y0, y1 = np.where(nan, 0, np.minimum(e, f)), np.where(nan, g - 1, np.maximum(e, f))
    nx = x1 - x0 + 1
    cnt = nx * (y1 - y0 + 1)
    assert cnt.sum() <= 1 << 25, "the library would halve G for this list"
    box = np.repeat(np.arange(n), cnt)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    nxr = np.repeat(nx, cnt)
    cid = (np.repeat(y0, cnt) + off // nxr) * g + np.repeat(x0, cnt) + off % nxr
    order = np.argsort(cid, kind="stable")        # ascending box index within every cell
    start = np.zeros(g * g + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(cid, minlength=g * g))
    return Index(g, invW, invH, start, box[order], boxes[box[order]])


@dataclass(frozen=True, eq=False)
class Walked:
    free: np.ndarray             # (S,) bool
    rows: np.ndarray             # (S,) cell rows of the span
    cols: np.ndarray
    run: np.ndarray              # (S, 2) entries of the runs of the first two rows (0 beyond the span)
    maxrun: np.ndarray           # (S,) the longest run of the span
    tail: np.ndarray             # (S,) a non-empty run of the span ends the box array
    hit_seg: np.ndarray          # one entry per (segment, listed box that meets it):
    hit_row: np.ndarray          # row of the span, from 0
    hit_pos: np.ndarray          # position in the run
    hit_len: np.ndarray          # length of that run

    def only(self, cond):
        """(S,) bool: blocked, and every hit satisfies cond (an array over the hits)."""
        S = len(self.free)
        bad = np.bincount(self.hit_seg[~cond], minlength=S)
        return ~self.free & (bad == 0)


def walk(ix: Index, segs, wrong=(), B=B_LDS) -> Walked:
    """The grid query of segs (S, 4) = (minx, miny, maxx, maxy) over ix, every listed box tested."""
    w = set(wrong)
    assert w <= set(SWITCHES)
    segs = np.ascontiguousarray(segs, F).reshape(-1, 4)
    S, g, T = len(segs), ix.g, len(ix.start)
    clamp = "e" not in w
    cx0, cx1 = cell(segs[:, 0], ix.invW, g, clamp), cell(segs[:, 2], ix.invW, g, clamp)
    cy0, cy1 = cell(segs[:, 1], ix.invH, g, clamp), cell(segs[:, 3], ix.invH, g, clamp)
    nrows = cy1 - cy0 + 1 - (1 if "d" in w else 0)
    if "a" in w:
        nrows = np.minimum(nrows, 2)
    free = np.ones(S, bool)
    run = np.zeros((S, 2), np.int64)
    maxrun = np.zeros(S, np.int64)
    tail = np.zeros(S, bool)
    hs, hr, hp, hl = [], [], [], []

    def disjoint(lhs, rhs, sw):
        with np.errstate(invalid="ignore"):
            return lhs < rhs if sw in w else lhs <= rhs

    for k in range(max(int(nrows.max()) if S else 0, 0)):
        act = np.flatnonzero(nrows > k)
        cy = cy0[act] + k
        a0 = cy * g + cx0[act]
        a1 = cy * g + cx1[act] + (0 if "c" in w else 1)
        ok = (a0 >= 0) & (a0 < T) & (a1 >= 0) & (a1 < T)
        b = np.where(ok, ix.start[np.clip(a0, 0, T - 1)], 0)
        L = np.maximum(np.where(ok, ix.start[np.clip(a1, 0, T - 1)], 0) - b, 0)
        if k < 2:
            run[act, k] = L
        maxrun[act] = np.maximum(maxrun[act], L)
        tail[act] |= (L > 0) & (b + L == ix.start[-1])
        n = np.maximum(L - 1, 0) if "g" in w else L
        if "b" in w:
            n = np.minimum(n, B)
        for j in range(int(n.max()) if len(n) else 0):
            sub = np.flatnonzero(n > j)
            o = ix.rows[b[sub] + j]
            s = segs[act[sub]]
            meets = ~(disjoint(s[:, 2], o[:, 0], "f0") | disjoint(o[:, 2], s[:, 0], "f1") |
                      disjoint(s[:, 3], o[:, 1], "f2") | disjoint(o[:, 3], s[:, 1], "f3"))
            h = sub[meets]
            free[act[h]] = False
            hs.append(act[h])
            hr.append(np.full(len(h), k))
            hp.append(np.full(len(h), j))
            hl.append(L[h])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return Walked(free, cy1 - cy0 + 1, cx1 - cx0 + 1, run, maxrun, tail, cat(hs), cat(hr), cat(hp), cat(hl))


def brute_free(boxes, segs, chunk=512) -> np.ndarray:
    """collisionCheck.cu:6-14 over every box in float32, NaN comparing false (as brute_free of
    tests/test_obstacle_grid.py, in chunks of segments)."""
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    segs = np.ascontiguousarray(segs, F).reshape(-1, 4)
    out = np.ones(len(segs), bool)
    o = boxes[None, :, :]
    for i in range(0, len(segs), chunk):
        s = segs[i:i + chunk, None, :]
        with np.errstate(invalid="ignore"):
            disjoint = (s[..., 2] <= o[..., 0]) | (o[..., 2] <= s[..., 0]) | (s[..., 3] <= o[..., 1]) | \
                       (o[..., 3] <= s[..., 1])
        out[i:i + chunk] = disjoint.all(axis=1)
    return out


def classes(wk: Walked, B) -> dict:
    """Masks over the segments of a correct walk, per class of the device walk with batch B."""
    first_hit = np.full(len(wk.free), 1 << 30)
    np.minimum.at(first_hit, wk.hit_seg, wk.hit_row)
    last_hit = np.full(len(wk.free), -1)
    np.maximum.at(last_hit, wk.hit_seg, wk.hit_row)
    hit = ~wk.free
    c = {"free": wk.free, "hit": hit}
    for r in range(1, 9):
        c[f"rows{r}"] = wk.rows == r
        c[f"cols{r}"] = wk.cols == r
    c["rows>=3"] = wk.rows >= 3                                  # the cy > cy0 reload
    c["odd-tail"] = (wk.rows >= 3) & (wk.rows % 2 == 1)          # the last pair's second row is empty (e1 = b1)
    c["hit-row3+"] = hit & (first_hit >= 2)                      # nothing met in the first pair of rows
    c["hit-last-row"] = hit & (wk.rows >= 2) & (first_hit == wk.rows - 1)
    c["hit-first-row"] = hit & (wk.rows >= 2) & (last_hit == 0)
    c["hit-odd-tail"] = c["odd-tail"] & c["hit-last-row"]
    c["empty-first-row"] = (wk.rows >= 2) & (wk.run[:, 0] == 0) & (wk.run[:, 1] > 0)
    for name, n in (("B-1", B - 1), ("B", B), ("B+1", B + 1), ("2B", 2 * B), ("2B+1", 2 * B + 1)):
        c[f"run={name}"] = wk.maxrun == n
    c["run>B"], c["run>2B"], c["run>4B"] = wk.maxrun > B, wk.maxrun > 2 * B, wk.maxrun > 4 * B
    c["hit-last-box"] = wk.only((wk.hit_pos == wk.hit_len - 1) & (wk.hit_len > 1))
    c["hit-first-box"] = wk.only((wk.hit_pos == 0) & (wk.hit_len > 1))
    c["hit-past-batch"] = wk.only(wk.hit_pos >= B)               # nothing met in any run's first batch
    c["hit-past-2-batches"] = wk.only(wk.hit_pos >= 2 * B)
    c["tail"] = wk.tail                                          # the batch runs on into the padding rows
    return c


def count(c: dict, name, verdict=None) -> int:
    m = c[name]
    if verdict is not None:
        m = m & c[verdict]
    return int(m.sum())


# ---------------------------------------------------------------- polylines
def lattice(v):
    """The nearest multiple of 1/64 (exact in float32 for |v| < 2^17)."""
    return F(np.round(np.float64(v) * 64.0) / 64.0)


class Poly:
    """A chain of point-agent rows; row 0 is the root."""

    def __init__(self, W, H, root=(1.0, 1.0)):
        self.W, self.H = float(W), float(H)
        self.pts = [(F(root[0]), F(root[1]))]
        self.ctl = [(F(0), F(0))]
        self.tags = [""]

    @staticmethod
    def _exact(c, t):
        return F(c + F(t - c)) == t

    def hop(self, x, y, tag="") -> int:
        """One row that ends on (x, y) exactly."""
        x, y = F(x), F(y)
        assert np.isfinite(x) and np.isfinite(y)
        cx, cy = self.pts[-1]
        assert self._exact(cx, x) and self._exact(cy, y), f"({cx}, {cy}) -> ({x}, {y}) rounds"
        self.pts.append((x, y))
        self.ctl.append((F(x - cx), F(y - cy)))
        self.tags.append(tag)
        return len(self.pts) - 1

    def goto(self, x, y, tag="") -> int:
        """Rows that end on (x, y) exactly: one where the hop is exact, else over lattice points."""
        x, y = F(x), F(y)
        cx, cy = self.pts[-1]
        if not (self._exact(cx, x) and self._exact(cy, y)):
            for wx, wy in ((lattice(cx), lattice(cy)), (lattice(x), lattice(y))):
                if (wx, wy) != self.pts[-1]:
                    self.hop(wx, wy, "via")
        return self.hop(x, y, tag)

    def seg(self, x0, y0, x1, y1, tag) -> int:
        """The segment (x0, y0) -> (x1, y1) as one row, both ends planted exactly."""
        self.goto(x0, y0, "to")
        return self.hop(x1, y1, tag)

    def walk(self, rng, rows, scales, tag="walk", p_out=0.0):
        """`rows` seeded hops over the 1/1024 lattice: (sx, sy) drawn from scales, reflected at
        the walls; with probability p_out a hop ends up to 0.5 outside and the next one returns."""
        q = lambda v: F(np.round(v * 1024.0) / 1024.0)
        x, y = self.pts[-1]
        if (q(x), q(y)) != (x, y):
            self.goto(q(x), q(y), "via")
        for _ in range(rows):
            x, y = (float(v) for v in self.pts[-1])
            inside = 0.0 < x < self.W and 0.0 < y < self.H
            sx, sy = scales[rng.integers(len(scales))]
            dx, dy = rng.uniform(-sx, sx), rng.uniform(-sy, sy)
            if inside and rng.random() < p_out:
                side = rng.integers(4)
                nx = (-rng.uniform(0.05, 0.5), self.W + rng.uniform(0.05, 0.5), x + dx, x + dx)[side]
                ny = (y + dy, y + dy, -rng.uniform(0.05, 0.5), self.H + rng.uniform(0.05, 0.5))[side]
                nx = min(max(nx, -0.5), self.W + 0.5)
                ny = min(max(ny, -0.5), self.H + 0.5)
            else:
                nx = x + dx if 0.03 <= x + dx <= self.W - 0.03 else min(max(x - dx, 0.03), self.W - 0.03)
                ny = y + dy if 0.03 <= y + dy <= self.H - 0.03 else min(max(y - dy, 0.03), self.H - 0.03)
            self.hop(q(nx), q(ny), tag)

    def case(self, name, boxes) -> Case:
        R = len(self.pts)
        assert R <= 8192, R
        state = np.zeros((R, 4), F)
        ctrl = np.zeros((R, 4), F)
        state[:, :2] = np.array(self.pts, F)
        ctrl[:, :2] = np.array(self.ctl, F)
        ctrl[1:, 2] = 1.0
        assert np.isfinite(state).all() and np.isfinite(ctrl).all()
        assert np.array_equal(state[:-1, :2] + ctrl[1:, :2], state[1:, :2])      # float32 adds: no row is STALE
        params = dict(numDisc=1, agentLength=1.0, width=self.W, height=self.H, agent="point")
        return Case(name, state, ctrl, np.arange(-1, R - 1, dtype=np.int32), np.ascontiguousarray(boxes, F), params)


@dataclass(frozen=True, eq=False)
class GridCase:
    case: Case
    g: int                       # the G the planner's rule gives this list
    tags: np.ndarray             # (R,) the builder's label of every row
    teeth: tuple = ()            # the switches this case is built to catch

    @property
    def name(self):
        return self.case.name

    @functools.cached_property
    def index(self) -> Index:
        ix = build_index(self.case.boxes, self.case.params["width"], self.case.params["height"])
        assert ix.g == self.g, (ix.g, self.g)
        return ix

    @functools.cached_property
    def segs(self) -> np.ndarray:
        """(R - 1, 4): the step box of rows 1 .. R - 1, min and max of the two stored states."""
        a, b = self.case.state[:-1, :2], self.case.state[1:, :2]
        return np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)

    @functools.cached_property
    def oob(self) -> np.ndarray:
        """(R - 1,) the row ends outside the workspace (statePropagator.cu:42-45): no box is looked at."""
        x, y = self.case.state[1:, 0], self.case.state[1:, 1]
        return (x <= 0) | (y <= 0) | (x >= F(self.case.params["width"])) | (y >= F(self.case.params["height"]))

    @functools.cached_property
    def outside_start(self) -> np.ndarray:
        x, y = self.case.state[:-1, 0], self.case.state[:-1, 1]
        out = (x <= 0) | (y <= 0) | (x >= F(self.case.params["width"])) | (y >= F(self.case.params["height"]))
        return out & ~self.oob

    @functools.cached_property
    def walked(self) -> Walked:
        return walk(self.index, self.segs)

    def bytes_of(self, free) -> np.ndarray:
        """The exported bytes of a chain whose rows' segments are `free` (R - 1,)."""
        own = np.where(self.oob | ~np.asarray(free, bool), BLOCKED, FREE).astype(np.uint8)
        dead_before = np.concatenate([[False], np.cumsum(own != FREE)[:-1] > 0])
        return np.concatenate([[FREE], np.where((own == FREE) & dead_before, FREE | CUT, own)]).astype(np.uint8)

    def tagged(self, prefix) -> np.ndarray:
        """(R - 1,) mask of the rows whose tag starts with prefix."""
        return np.array([t.startswith(prefix) for t in self.tags[1:]], bool)


def _fillers(rng, count, W, H, keep_out, hmax=0.1):
    """`count` seeded boxes inside the workspace, none touching a rectangle of keep_out."""
    out = []
    while len(out) < count:
        cx, cy = rng.uniform(0.3, W - 0.3), rng.uniform(0.3, H - 0.3)
        hx, hy = rng.uniform(0.02, hmax, 2)
        b = (cx - hx, cy - hy, cx + hx, cy + hy)
        if all(b[2] < k[0] or k[2] < b[0] or b[3] < k[1] or k[3] < b[1] for k in keep_out):
            out.append(b)
    return out


NAN_BOX = (NAN, 17.0, 1.0, 17.5)       # meets a segment with minx < 1 whose y range meets (17, 17.5)


# ---- spans: G = 16 on 20 x 20, cells of 1.25
@functools.lru_cache(maxsize=None)
def spans(nan=False) -> GridCase:
    W = H = 20.0
    rng = np.random.default_rng(101)
    t1, t2 = (2.625, 2.625, 2.75, 2.75), (12.25, 12.25, 12.375, 12.375)      # in cells (2, 2) and (9, 9)
    boxes = [t1, t2] + _fillers(rng, 478, W, H, [(2.2, 2.2, 12.8, 12.8)])
    if nan:
        boxes[2] = NAN_BOX
    assert planner_g(len(boxes)) == 16
    p = Poly(W, H)
    lo = lambda c, off: c * 1.25 + off
    for R in range(1, 9):
        for C in range(1, 9):
            for v in range(2):
                d = v * 0.03125
                ex, ey = lo(2 + C - 1, 0.5 + d), lo(2 + R - 1, 0.5 + d)         # far end, seen from cell (2, 2)
                p.seg(2.6875 + d, 2.6875 + d, ex, ey, f"span:first:{R}x{C}")     # starts inside t1
                p.seg(2.875 + d, 2.875 + d, ex, ey, f"span:free:{R}x{C}")        # starts beside t1
                fx, fy = lo(9 - C + 1, 0.75 - d), lo(9 - R + 1, 0.75 - d)        # far end, seen from cell (9, 9)
                p.seg(fx, fy, 12.3125 - d, 12.3125 - d, f"span:last:{R}x{C}")    # ends inside t2
                p.seg(fx, fy, 12.125 - d, 12.125 - d, f"span:free:{R}x{C}")      # ends beside t2
    p.walk(rng, 1500, [(0.1, 0.1), (0.5, 0.5), (3.0, 3.0), (0.05, 6.0), (6.0, 0.05)], p_out=0.02)
    return GridCase(p.case("spans-nan" if nan else "spans", boxes), 16, np.array(p.tags), teeth=("a", "c", "d"))


# ---- runs, tail: G = 8 on 20 x 20, cells of 2.5; a cell's boxes stand side by side, 1/32 wide at a
# pitch of 1/16, in ascending box order
RUN_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 16, 17, 33, 2, 6, 12)    # the last three only fill the list up to G = 8
RUN_CELLS = [(cx, cy) for cy in (1, 3, 5, 7) for cx in (1, 3, 5, 7)]


def _cell_boxes(cx, cy, k):
    x0, y0 = cx * 2.5 + 0.125, cy * 2.5 + 1.0
    return [(x0 + i / 16, y0, x0 + i / 16 + 1 / 32, y0 + 0.25) for i in range(k)]


def _cell_queries(p, cx, cy, k, tag, reps=16, first=0):
    """Short segments inside cell (cx, cy): beside its boxes, inside box `first` alone, inside box k - 1 alone."""
    x0, y0 = cx * 2.5 + 0.125, cy * 2.5 + 1.0
    for v in range(reps):
        y = y0 + (v + 1) / 128
        p.seg(x0 + 5 / 128, y, x0 + 7 / 128, y + 1 / 64, f"{tag}:free")          # the gap behind box 0
        if k > first:
            p.seg(x0 + first / 16 + 1 / 128, y, x0 + first / 16 + 3 / 128, y + 1 / 64, f"{tag}:first")
            p.seg(x0 + (k - 1) / 16 + 3 / 128, y + 1 / 64, x0 + (k - 1) / 16 + 1 / 128, y, f"{tag}:last")


def _cell_columns(p, cx, cy, k, tag, reps=4, first=0):
    """Thin segments from the empty cell row below into the cell (an empty first row, a populated
    second one) and from the cell into the empty row above."""
    x0, y0 = cx * 2.5 + 0.125, cy * 2.5 + 1.0
    for v in range(reps):
        d = v / 256
        for xa, kind in ((x0 + 5 / 128, "free"), (x0 + (k - 1) / 16 + 1 / 128, "last"), (x0 + first / 16 + 1 / 128, "first")):
            if kind != "free" and k <= first:
                continue
            p.seg(xa + d, cy * 2.5 - 0.5, xa + d + 1 / 128, y0 + 0.125, f"{tag}:below:{kind}")
            p.seg(xa + d + 1 / 128, y0 + 0.125, xa + d, cy * 2.5 + 3.0, f"{tag}:above:{kind}")


@functools.lru_cache(maxsize=None)
def runs(nan=False) -> GridCase:
    """Cells whose run is exactly RUN_LENGTHS, each with eight empty neighbours.  nan: box 0 is a
    NaN box, listed first in every cell, and every cell holds one crafted box fewer."""
    W = H = 20.0
    rng = np.random.default_rng(102)
    extra = 1 if nan else 0
    boxes = [NAN_BOX] if nan else []
    for (cx, cy), k in zip(RUN_CELLS, RUN_LENGTHS):
        boxes += _cell_boxes(cx, cy, max(k - extra, 0))
    assert planner_g(len(boxes)) == 8, len(boxes)
    p = Poly(W, H)
    for (cx, cy), k in zip(RUN_CELLS, RUN_LENGTHS):
        _cell_queries(p, cx, cy, max(k - extra, 0), f"run{k}")
        _cell_columns(p, cx, cy, max(k - extra, 0), f"run{k}")
    p.walk(rng, 800, [(0.1, 0.1), (0.6, 0.6), (4.0, 0.3), (0.3, 4.0)])
    return GridCase(p.case("runs-nan" if nan else "runs", boxes), 8, np.array(p.tags), teeth=("b", "g"))


TAIL_LENGTHS = (1, 3, 4, 5, 7, 8, 9)       # 1, B - 1, B, B + 1 for B = 4 and B = 8


@functools.lru_cache(maxsize=None)
def tail(k) -> GridCase:
    """The last cell (7, 7) lists exactly k boxes, the end of the box array; 2, 3 and 5 in the other corners."""
    W = H = 20.0
    rng = np.random.default_rng(110 + k)
    corners = (((7, 7), k), ((0, 0), 2), ((7, 0), 3), ((0, 7), 5))
    boxes = _fillers(rng, 100, W, H, [(0, 0, 2.8, 2.8), (17.2, 0, 20, 2.8), (0, 17.2, 2.8, 20), (17.2, 17.2, 20, 20)])
    for (cx, cy), n in corners:
        boxes += _cell_boxes(cx, cy, n)
    assert planner_g(len(boxes)) == 8
    p = Poly(W, H)
    for (cx, cy), n in corners:
        _cell_queries(p, cx, cy, n, f"corner{cx}{cy}")
    x0, y0 = 7 * 2.5 + 0.125, 7 * 2.5 + 1.0
    for v in range(32):                     # across the last cell: from (6, 6), (7, 6) and (6, 7), and from outside
        d = v / 2048
        for sx, sy, frm in ((16.0, 16.0, "66"), (x0 + 5 / 128, 16.0, "76"), (16.0, y0 + 0.125, "67"),
                            (20.25, y0 + 0.125, "east"), (x0 + 5 / 128, 20.25, "north")):
            free_x, last_x = x0 + 5 / 128 + d, x0 + (k - 1) / 16 + 1 / 128 + d
            if frm in ("67", "east"):       # a level segment: the free one stays under the boxes
                p.seg(sx, y0 - 0.25 + d, free_x, y0 - 0.125, f"across{frm}:free")
            else:
                p.seg(sx, sy, free_x, y0 + 0.125, f"across{frm}:free")
            p.seg(sx, sy + d, last_x, y0 + 0.125, f"across{frm}:hit")
    p.walk(rng, 300, [(0.1, 0.1), (0.6, 0.6), (4.0, 0.3), (0.3, 4.0)], p_out=0.05)
    return GridCase(p.case(f"tail-{k}", boxes), 8, np.array(p.tags))


# ---- lines: G = 8; the cell lines of 20 x 20 are 2.5 k, of 30 x 12 they are 3.75 k and 1.5 k
def line_floats(k, extent, g=8):
    """(p, t): t the smallest float whose cell is >= k, p the float below it.  t is below the line
    k * extent / g where v * inv rounds up onto k (fl(8 / 30) * 3.7499998 = 1 in float32)."""
    inv = F(g) / F(extent)
    t = F(k * extent / g)
    while cell(down(t), inv, g) >= k:
        t = down(t)
    while cell(t, inv, g) < k:
        t = up(t)
    return down(t), t


@functools.lru_cache(maxsize=None)
def lines(W=20.0, H=20.0) -> GridCase:
    rng = np.random.default_rng(103)
    boxes = []
    band = (0.5, 1.0)                       # the x-line boxes lie in this y band, the y-line boxes in this x band
    for k in range(1, 8):
        for axis, extent in ((0, W), (1, H)):
            pk, tk = line_floats(k, extent)
            lohi = (tk, tk + F(0.25)) if k % 2 else (tk - F(0.25), pk)     # odd k: from t up; even k: up to p
            boxes.append((lohi[0], band[0], lohi[1], band[1]) if axis == 0 else (band[0], lohi[0], band[1], lohi[1]))
    yb, xb = 0.45 * H, 0.45 * W
    boxes += [(0.25, yb, 0.5, yb + 0.5), (W - 0.5, yb, W - 0.25, yb + 0.5),              # beside the four walls
              (xb, 0.25, xb + 0.5, 0.5), (xb, H - 0.5, xb + 0.5, H - 0.25),
              (0.25, 0.25, 0.4375, 0.4375), (W - 0.4375, H - 0.4375, W - 0.25, H - 0.25),  # cells (0, 0) and (7, 7)
              (6.0, 6.0, 4.0, 8.0), (7.5, 7.5, 7.5, 7.5), (-INF, 10.0, INF, 10.5)]        # inverted, zero area, infinite
    boxes += _fillers(rng, 85, W, H, [(0, 0, W, 1.2), (0, 0, 1.2, H), (0, H - 1.2, W, H), (W - 1.2, 0, W, H),
                                      (3.0, 5.5, 9.0, 11.0)])
    assert planner_g(len(boxes)) == 8
    p = Poly(W, H)
    for k in range(1, 8):
        for axis, extent in ((0, W), (1, H)):
            pk, tk = line_floats(k, extent)
            for v in range(4):
                o0, o1 = 0.625 + v / 64, 0.75 + v / 64                 # inside the band on the other axis
                for e in (down(pk), pk, tk, up(tk), up(up(tk))):
                    far = F(e - F(0.125)) if k % 2 else F(e + F(0.125))   # the planted float is maxx (odd k) or minx
                    pts = (far, o0, e, o1) if k % 2 else (e, o0, far, o1)
                    if axis == 1:
                        pts = (pts[1], pts[0], pts[3], pts[2])
                    p.seg(*pts, f"line:{'xy'[axis]}{k}")
    for v in range(16):
        d, e = v / 64, v / 128
        for hit in (True, False):
            y = yb + 0.125 + d / 2 if hit else yb - 0.5 - d / 2
            x = xb + 0.125 + d / 2 if hit else xb - 0.5 - d / 2
            p.seg(-0.5, y, 0.75, y + e, "outside:west")
            p.seg(W + 0.5, y, W - 0.75, y + e, "outside:east")
            p.seg(x, -0.5, x + e, 0.75, "outside:south")
            p.seg(x, H + 0.5, x + e, H - 0.75, "outside:north")
        p.seg(-0.5, 0.3 + e, 0.75, 0.3125 + e, "outside:row0")                     # from the west into cell (0, 0)
        p.seg(-0.25, -0.25, 0.3 + e, 0.3125 + e, "outside:corner")
        p.seg(W + 0.5, H - 0.3 - e, W - 0.75, H - 0.3125 - e, "outside:rowG")      # from the east into cell (7, 7)
        p.seg(W + 0.25, H + 0.25, W - 0.3 - e, H - 0.3125 - e, "outside:corner")
        p.seg(3.5 + e, 7.0, 6.5, 7.0 + e, "odd:inverted-hit")                      # minx < 4 and maxx > 6
        p.seg(4.5 + e, 7.0, 5.5, 7.0 + e, "odd:inverted-free")
        p.seg(7.4375 + e / 4, 7.4375, 7.5625, 7.5625 + e / 4, "odd:zero-hit")
        p.seg(7.5, 7.4375 + e / 4, 7.5625, 7.5625, "odd:zero-touch")               # o.z <= minx at equality
        p.seg(12.0 + d, 9.875, 12.0 + d + e, 10.125, "odd:inf-hit")
        p.seg(12.0 + d, 9.75, 12.0 + d + e, 10.0, "odd:inf-touch")                 # maxy <= o.y at equality
    p.walk(rng, 600, [(0.1, 0.1), (0.6, 0.6), (4.0, 0.3), (0.3, 4.0)], p_out=0.05)
    name = "lines" if (W, H) == (20.0, 20.0) else f"lines-{W:g}x{H:g}"
    return GridCase(p.case(name, boxes), 8, np.array(p.tags), teeth=("e", "f0", "f1", "f2", "f3"))


# ---- G = 1 and the clamp at G = 90
@functools.lru_cache(maxsize=None)
def g1() -> GridCase:
    p = Poly(20.0, 20.0)
    p.walk(np.random.default_rng(104), 1000, [(0.2, 0.2), (1.0, 1.0), (6.0, 6.0), (0.1, 8.0)], p_out=0.05)
    return GridCase(p.case("g1", [(8.0, 8.0, 12.0, 12.0), (3.0, 14.0, 5.0, 15.0)]), 1, np.array(p.tags))


def dense_boxes(W=20.0, H=20.0, root=(10.0, 10.0), planted=None) -> np.ndarray:
    """16,000 boxes of half-size up to 0.06: grid_resolution gives 90 (2 * 89^2 = 15,842 < 16,000)."""
    return random_boxes(16000, W, H, 21, 0.06, 0.3, planted=planted, root=root + (0.0, 0.0))


@functools.lru_cache(maxsize=None)
def g90(W=20.0, H=20.0) -> GridCase:
    assert resolution(16000) == 90 and resolution(15842) == 89
    p = Poly(W, H, root=(W / 2, H / 2))
    p.walk(np.random.default_rng(105), 8000, [(0.04, 0.04), (0.12, 0.12), (0.02, 1.5), (1.5, 0.02), (0.01, 0.7),
                                              (0.7, 0.01), (1.0, 1.0)], p_out=0.02)
    name = "g90" if (W, H) == (20.0, 20.0) else f"g90-{W:g}x{H:g}"
    return GridCase(p.case(name, dense_boxes(W, H, (W / 2, H / 2))), 90, np.array(p.tags))


def polyline_cases() -> list:
    out = [("spans", spans), ("runs", runs)]
    out += [(f"tail-{k}", functools.partial(tail, k)) for k in TAIL_LENGTHS]
    out += [("lines", lines), ("lines-30x12", functools.partial(lines, 30.0, 12.0)), ("g1", g1), ("g90", g90),
            ("g90-30x12", functools.partial(g90, 30.0, 12.0)),
            ("spans-nan", functools.partial(spans, True)), ("runs-nan", functools.partial(runs, True))]
    return out


POLYLINES = polyline_cases()
POLYLINE_IDS = [i for i, _ in POLYLINES]


# ---------------------------------------------------------------- planner scenarios
POINT = dict(agent="point", numDisc=1, numIterations=4)
CLUSTER_ROOT = (10.2, 10.3)
CLUSTERS = ((9, (0.45, 0.1)), (17, (-0.2, 0.5)), (33, (-0.4, -0.45)), (9, (0.1, -0.7)), (17, (0.7, 0.6)),
            (33, (0.85, -0.3)))             # boxes, offset of the cluster's patch from the root


def cluster_boxes() -> np.ndarray:
    """3,000 background boxes (G = 40, cells of 0.5) and clusters of 9, 17 and 33 boxes of 0.02 x 0.02
    on a 0.12 x 0.12 patch each, 0.3 to 1.0 from the root."""
    rng = np.random.default_rng(106)
    bg = random_boxes(3000, 20.0, 20.0, 23, 0.05, 0.25, root=CLUSTER_ROOT + (0.0, 0.0))
    rows = []
    for n, (ox, oy) in CLUSTERS:
        assert 0.3 <= np.hypot(ox, oy) <= 1.0
        c = np.stack([CLUSTER_ROOT[0] + ox + rng.uniform(0.0, 0.1, n), CLUSTER_ROOT[1] + oy + rng.uniform(0.0, 0.1, n)], 1)
        rows.append(np.concatenate([c, c + 0.02], axis=1))
    return np.concatenate([bg] + rows).astype(F)


def _planner_scenarios() -> list:
    S = []

    def add(name, kw, boxes, initial, goal=(2.0, 18.0), **rest):
        S.append(Scenario(name=name, family="P", targets="the grid walk at long segments", kw=kw, boxes=boxes,
                          initial=initial, goal=goal, obstacle_form="grid", **rest))

    centre = (10.0, 10.0, 0.0, 0.0)
    two = {"SBMP_STEP": "0"}
    add("P-g90-point", POINT, dense_boxes, centre)
    add("P-g90-point-two-launch", POINT, dense_boxes, centre, env=two)
    add("P-g90-point-group2", POINT, dense_boxes, centre, local_group=2)
    add("P-g90-n16", dict(POINT, n=16), dense_boxes, centre)
    add("P-g90-n16-group8", dict(POINT, n=16), dense_boxes, centre, local_group=8)
    add("P-clusters", dict(POINT, numIterations=5), cluster_boxes, CLUSTER_ROOT + (0.0, 0.0))
    add("P-clusters-two-launch", dict(POINT, numIterations=5), cluster_boxes, CLUSTER_ROOT + (0.0, 0.0), env=two)
    car = dict(numDisc=2, numIterations=4)
    car_root = (4.0, 10.0, 0.05, 12.0)      # the E root of tests/edge_scenarios.py
    car_boxes = lambda: random_boxes(3000, 20.0, 20.0, 11, 0.08, 0.5, root=car_root)
    add("P-fast-car", car, car_boxes, car_root)
    add("P-fast-car-two-launch", car, car_boxes, car_root, env=two)
    wide = dict(POINT, width=30.0, height=12.0)
    add("P-g90-30x12", wide, lambda: dense_boxes(30.0, 12.0, (15.0, 6.0)), (15.0, 6.0, 0.0, 0.0), goal=(27.0, 10.0))
    add("P-g90-nan", POINT, lambda: dense_boxes(planted=(NAN, 3.0, 9.0, 3.4)), centre)
    # the root in the last cell but one: children walk cell (89, 89), whose run ends build_grid's box array
    add("P-g90-corner", POINT, lambda: dense_boxes(root=(19.7, 19.7)), (19.7, 19.7, 0.0, 0.0))
    return S


SCENARIOS = _planner_scenarios()
SCENARIO_IDS = [s.name for s in SCENARIOS]
BY_NAME = {s.name: s for s in SCENARIOS}


def batch_of(sc: Scenario) -> int:
    """Boxes per batch of the walk a scenario's step form runs (the NaN list: the batched form's 8)."""
    return B_GLOBAL if sc.step_form == "two-launch" and "nan" not in sc.name else B_LDS


@dataclass(frozen=True, eq=False)
class Steps:
    segs: np.ndarray             # (S, 4) step boxes whose end lies inside the workspace (the others walk nothing)
    iterations: int


@functools.lru_cache(maxsize=None)
def steps(name) -> Steps:
    """Every slot's segment of every iteration of scenario `name`, valid or not, from the stepped
    oracle.  Point, numDisc = 1: parent -> child.  Car: the Euler steps, each replayed on its own by
    the oracle (one step of duration dt from the state the step before it left)."""
    from oracle.pyoracle import lib, replay
    from tree_recheck_model import planner_config
    sc = BY_NAME[name]
    cfg, extra = sc.config()
    W, H = F(cfg["width"]), F(cfg["height"])
    o = make_oracle(sc, plan=False)
    slots = lib().oracle_num_slots(o._h)
    out, its = [], 0
    while o.step():
        its += 1
        u, up_ = o.unexplored()
        u, up_ = u[:slots], up_[:slots]
        tree = o.tree()[0]
        live = (up_ >= 0) & (up_ < o.info()["treeSize"])
        par = tree[np.where(live, up_, 0), :4]
        if extra.get("agent", "car") == "point":
            a, b = par[live, :2], u[live, :2]
            inside = (b[:, 0] > 0) & (b[:, 1] > 0) & (b[:, 0] < W) & (b[:, 1] < H)
            out.append(np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)[inside])
            continue
        D = cfg["numDisc"]
        pc = planner_config(numDisc=1, agentLength=cfg["agentLength"], width=cfg["width"], height=cfg["height"])
        ctl = u[live, 4:7].copy()
        ctl[:, 2] = ctl[:, 2] / F(D)                # dt = duration / numDisc in float32
        cur, alive = par[live].copy(), np.ones(int(live.sum()), bool)
        for _ in range(D):
            nxt, v = replay(pc, sc.obstacles(), cur, ctl)
            inside = (nxt[:, 0] > 0) & (nxt[:, 1] > 0) & (nxt[:, 0] < W) & (nxt[:, 1] < H)
            a, b = cur[:, :2], nxt[:, :2]
            out.append(np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)[alive & inside])
            cur, alive = nxt, alive & v
        assert np.array_equal(cur[alive].view(np.uint32), u[live, :4][alive].view(np.uint32))   # the replayed steps are the plan's
    return Steps(np.concatenate(out), its)


def scenario_steps(sc: Scenario) -> Steps:
    return steps(sc.name)

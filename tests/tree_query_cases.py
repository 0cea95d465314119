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

A masked case (masked_case()) is the same plus a mask of R bytes for k_tree_query_alive
(sbmp_tree_query_alive_batch): a row is skipped iff its byte is 0.  It also carries `differs`
= [(goal, field), ...]: where the unmasked model's answer must differ from the masked one,
asserted when the case is built, so that no case goes vacuous.  The masked kernel takes one
row per lane and sweep, 256 rows per workgroup, on a grid of at most 8 workgroups per CU: one
sweep is at most SWEEP = 256 x 8 x 256 = 524,288 rows on an MI355X (fewer resident workgroups
only shorten it), and the two largest masked cases go round its grid-stride loop a second and a
third time.
"""
from __future__ import annotations

import collections
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
    # Row 211 lies exactly on the kernel's threshold: its d2 is t(r3), the largest d2 with
    # sqrt(d2) < r3, because the next float above d2 already has the greater square root r3.  (Of
    # row k's d2 this need not hold: some neighbouring d2 share a square root.)  d2 <= t takes the
    # row, d2 < t would not; r4 = sqrt(d2) itself leaves it outside.
    one = np.float32(1.0)
    for j in range(64):
        x = np.float32(30.3 + j / 1024.0)
        e2 = d2_of(np.array([x]), np.array([np.float32(10.0)]), 30.0, 10.0)[0]
        r4, r3 = np.sqrt(e2, dtype=np.float32), np.sqrt(np.nextafter(e2, one), dtype=np.float32)
        if r3 > r4:
            break
    assert r3 > r4 and np.sqrt(e2, dtype=np.float32) < r3
    _plant(state, ctrl, 211, x, 10.0, 5.0)
    goals = [(10.0, 10.0, d), (10.0, 10.0, up), (10.0, 10.0, down), (30.0, 10.0, r3), (30.0, 10.0, r4)]
    expect = [(0, "count", 2), (0, "bestRow", 20), (1, "count", 3), (1, "bestRow", k), (2, "count", 2),
              (2, "bestRow", 20), (0, "firstRow", 20), (1, "firstRow", 20), (2, "firstRow", 20),
              (3, "count", 1), (3, "bestRow", 211), (3, "nearestRow", 211), (4, "count", 0), (4, "nearestRow", 211),
              (4, "nearestDistance", r4)]
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


def tiles(Q: int):
    """Q goals over 5,000 rows, each with one inside row in a full chunk of k_tree_query (rows
    [0, 2048) and [2048, 4096), by turns) and a cheaper, farther one in the tail chunk [4096, 5000):
    every tile that takes part runs query_rows<NG, false> and <NG, true> on several workgroups."""
    R = 5000
    state, ctrl = background(R)
    goals, expect = [], []
    for q in range(Q):
        cx, cy = 10.0 + 8.0 * (q % 6), 10.0 + 8.0 * (q // 6)
        full, tail = (q % 2) * 2048 + 100 + 97 * q, 4096 + 13 + 47 * q
        assert full < (q % 2 + 1) * 2048 and 4096 <= tail < R
        _plant(state, ctrl, full, cx + 0.125, cy, 3.0 + q)
        _plant(state, ctrl, tail, cx, cy + 0.25, 1.0 + 0.0625 * q)
        goals.append((cx, cy, 0.5))
        expect += [(q, "count", 2), (q, "firstRow", full), (q, "bestRow", tail), (q, "nearestRow", full),
                   (q, "bestCost", np.float32(1.0 + 0.0625 * q)), (q, "nearestDistance", np.float32(0.125))]
    return state, ctrl, goals, expect


# rows of the non-finite cases: (row, x, y, cost, alive).  Goal 0 is (10, 10, 0.5), goal 1 (40, 10, 0.5).
_NONFINITE = ((10, 10.25, 10.0, 3.0, 1),            # finite, inside goal 0
              (20, np.nan, 10.0, 0.0, 1),            # x = NaN, the cheapest row there is
              (30, 10.0, np.inf, 0.0, 1),            # y = +inf
              (40, np.nan, 10.0, 0.0, 0),
              (50, 10.0, np.inf, 0.0, 0),
              (300, 10.125, 10.0, np.inf, 1),        # inside goal 0 and nearer, cost +inf: counts, loses bestRow
              (310, 10.0625, 10.0, np.inf, 0),
              (400, 40.125, 10.0, np.inf, 1),        # the only alive inside row of goal 1
              (410, 40.0625, 10.0, 2.0, 0))          # a dead finite one beside it


def _nonfinite_rows():
    R = 600
    state, ctrl = background(R)
    mask = np.ones(R, np.uint8)
    for row, x, y, cost, alive in _NONFINITE:
        _plant(state, ctrl, row, x, y, cost)
        mask[row] = alive
    goals = [(10.0, 10.0, 0.5), (40.0, 10.0, 0.5), (10.0, 10.0, np.inf), (500.0, 900.0, 1.0)]
    return state, ctrl, goals, mask


def nonfinite():
    """The rows of masked-nonfinite without the mask: a row with x = NaN or y = +inf is never
    inside (not even r = +inf takes it) and never nearest; an inside row of cost +inf counts and
    loses bestRow to any finite cost."""
    state, ctrl, goals, _ = _nonfinite_rows()
    R = len(state)
    expect = [(0, "count", 3), (0, "firstRow", 10), (0, "bestRow", 10), (0, "bestCost", np.float32(3.0)),
              (0, "nearestRow", 310), (0, "nearestDistance", np.float32(0.0625)),
              (1, "count", 2), (1, "bestRow", 410), (1, "nearestRow", 410),
              (2, "count", R - 4), (2, "firstRow", 0), (2, "nearestRow", 310),
              (3, "count", 0)]
    return state, ctrl, goals, expect


TILE_COUNTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 18)

BUILDERS = {f"single-{R}": functools.partial(single, R) for R in ROW_COUNTS}
BUILDERS.update({"ties": ties, "radius-edges": radius_edges, "zero-distance": zero_distance,
                 "degenerate": degenerate, "overflow": overflow, "random": random_rows})
BUILDERS.update({f"goals-{Q}": functools.partial(goal_count, Q) for Q in GOAL_COUNTS})
BUILDERS.update({f"tiles-{Q}": functools.partial(tiles, Q) for Q in TILE_COUNTS})
BUILDERS["nonfinite"] = nonfinite
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


# ---------------------------------------------------------------- masked cases
SWEEP = 256 * 8 * 256   # rows of one sweep of k_tree_query_alive's grid on an MI355X, at most
MASKED_ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, SWEEP + 77, 2 * SWEEP + 1)
MASKED_GOAL_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 65)
ALIVE_BYTES = (1, 2, 0x7f, 0x80, 0xff)
ONE_ROW_TREE = 700       # masked-one-*: three workgroups of the masked kernel
ONE_ROWS = (0, 255, 256, ONE_ROW_TREE - 1)

MaskedCase = collections.namedtuple("MaskedCase", "name state ctrl goals mask expect differs model unmasked")


def _empty_expect(q):
    return [(q, "count", 0), (q, "firstRow", -1), (q, "bestRow", -1), (q, "bestCost", np.float32(0.0)),
            (q, "nearestRow", -1), (q, "nearestDistance", np.float32(np.inf))]


def masked_ties():
    R = 5000   # 20 workgroups of 256 rows
    state, ctrl = background(R)
    mask = np.ones(R, np.uint8)
    dead = []
    # goal 0: three rows of equal d2 (0.25 from the centre) in three workgroups, the lowest dead
    _plant(state, ctrl, 7, 30.25, 10.0, 9.0)
    _plant(state, ctrl, 300, 29.75, 10.0, 4.0)
    _plant(state, ctrl, R - 2, 30.0, 10.25, 5.0)
    dead.append(7)
    # goal 1: three inside rows of equal cost, the lowest dead
    _plant(state, ctrl, 5, 10.125, 10.0, 2.5)
    _plant(state, ctrl, 600, 10.0, 10.25, 2.5)
    _plant(state, ctrl, R - 1, 10.25, 10.0, 2.5)
    dead.append(5)
    # goal 2: rows 3 and 4100 identical, row 3 dead; row 2000 dearer and farther
    _plant(state, ctrl, 3, 50.125, 10.0, 1.5)
    _plant(state, ctrl, 4100, 50.125, 10.0, 1.5)
    _plant(state, ctrl, 2000, 50.25, 10.25, 6.0)
    dead.append(3)
    # goal 3: the cheapest inside row dead, a dearer one alive (and nearer, so nearestRow stays)
    _plant(state, ctrl, 50, 10.25, 30.0, 1.0)
    _plant(state, ctrl, 900, 10.125, 30.0, 4.0)
    dead.append(50)
    # goal 4: the only inside row dead; the nearest alive row lies outside the disc
    _plant(state, ctrl, 1500, 30.125, 30.0, 2.0)
    _plant(state, ctrl, 1600, 30.75, 30.0, 2.0)
    dead.append(1500)
    # goal 5: the root inside and dead
    _plant(state, ctrl, 0, 50.125, 30.0, 0.0)
    _plant(state, ctrl, 100, 50.0, 30.25, 0.5)
    dead.append(0)
    mask[dead] = 0
    goals = [(30.0, 10.0, 0.5), (10.0, 10.0, 0.5), (50.0, 10.0, 0.5), (10.0, 30.0, 0.5), (30.0, 30.0, 0.5),
             (50.0, 30.0, 0.5)]
    expect = [(0, "count", 2), (0, "nearestRow", 300), (0, "nearestDistance", np.float32(0.25)), (0, "bestRow", 300),
              (1, "count", 2), (1, "firstRow", 600), (1, "bestRow", 600), (1, "bestCost", np.float32(2.5)),
              (2, "count", 2), (2, "firstRow", 2000), (2, "bestRow", 4100), (2, "nearestRow", 4100),
              (3, "count", 1), (3, "bestRow", 900), (3, "bestCost", np.float32(4.0)), (3, "nearestRow", 900),
              (4, "count", 0), (4, "firstRow", -1), (4, "bestRow", -1), (4, "bestCost", np.float32(0.0)),
              (4, "nearestRow", 1600), (4, "nearestDistance", np.float32(0.75)),
              (5, "count", 1), (5, "firstRow", 100), (5, "bestRow", 100), (5, "nearestRow", 100)]
    differs = [(0, "nearestRow"), (0, "count"), (1, "bestRow"), (1, "firstRow"), (2, "bestRow"), (2, "nearestRow"),
               (2, "firstRow"), (3, "bestRow"), (3, "bestCost"), (4, "count"), (4, "bestRow"), (4, "nearestRow"),
               (5, "firstRow"), (5, "bestRow"), (5, "nearestRow")]
    return state, ctrl, goals, mask, expect, differs


def masked_radius_edges():
    """radius_edges with the edge row alive and a dead twin of it at a lower row."""
    state, ctrl, goals, expect = radius_edges()
    k, twin = 137, 60
    state, ctrl = state.copy(), ctrl.copy()
    state[twin], ctrl[twin] = state[k], ctrl[k]
    mask = np.ones(len(state), np.uint8)
    mask[twin] = 0
    return state, ctrl, goals, mask, expect, [(1, "count"), (1, "bestRow")]


def masked_zero_distance():
    """zero_distance with the row on the centre alive and a dead twin of it at a lower row."""
    state, ctrl, goals, expect = zero_distance()
    state, ctrl = state.copy(), ctrl.copy()
    state[100], ctrl[100] = state[200], ctrl[200]
    mask = np.ones(len(state), np.uint8)
    mask[100] = 0
    return state, ctrl, goals, mask, expect, [(0, "count"), (0, "firstRow"), (0, "bestRow"), (0, "nearestRow")]


def _scattered_mask(R, seed):
    return (np.random.default_rng(seed).random(R) < 0.5).astype(np.uint8)


def masked_bytes():
    """Alive bytes drawn from ALIVE_BYTES, dead = 0, over the scattered rows of goals-9: the
    answers are those of the same mask written as 0 / 1 (masked_case("masked-bytes-01"))."""
    state, ctrl, goals, _ = goal_count(9)
    rng = np.random.default_rng(31)
    mask = _scattered_mask(len(state), 30) * rng.choice(np.array(ALIVE_BYTES, np.uint8), size=len(state))
    assert set(np.unique(mask).tolist()) == {0, *ALIVE_BYTES}
    return state, ctrl, goals, mask.astype(np.uint8), [], [(q, "count") for q in range(9)]


def masked_bytes_01():
    state, ctrl, goals, mask, expect, differs = masked_bytes()
    return state, ctrl, goals, (mask != 0).astype(np.uint8), expect, differs


def _thirteen_goals(R):
    """13 goals over background(R) (a call of the tiles 8, 4 and 1), each with one planted inside row."""
    state, ctrl = background(R)
    goals, rows = [], []
    for q in range(13):
        cx, cy = 10.0 + 8.0 * (q % 5), 10.0 + 8.0 * (q // 5)
        row = (23 * q + 7) % R
        _plant(state, ctrl, row, cx + 0.125, cy, 2.0 + q)
        goals.append((cx, cy, 0.5))
        rows.append(row)
    assert len(set(rows)) == 13
    return state, ctrl, goals, rows


def masked_none():
    """No alive row: the empty-set answer for every goal, in every tile of a 13-goal call."""
    R = 300
    state, ctrl, goals, _ = _thirteen_goals(R)
    expect = [e for q in range(13) for e in _empty_expect(q)]
    differs = [(q, f) for q in range(13) for f in ("count", "firstRow", "bestRow", "bestCost", "nearestRow",
                                                   "nearestDistance")]
    return state, ctrl, goals, np.zeros(R, np.uint8), expect, differs


def masked_one(p: int):
    """Exactly one alive row, p, which is inside goal 0 only; the other twelve goals' planted
    rows are dead, so each of them answers count 0 and nearestRow p."""
    R = ONE_ROW_TREE
    state, ctrl, goals, rows = _thirteen_goals(R)
    assert p not in rows[1:]
    if p != rows[0]:
        state[p], ctrl[p] = state[rows[0]], ctrl[rows[0]]   # a twin of goal 0's planted row
    mask = np.zeros(R, np.uint8)
    mask[p] = 1
    expect = [(0, "count", 1), (0, "firstRow", p), (0, "bestRow", p), (0, "bestCost", np.float32(2.0)),
              (0, "nearestRow", p), (0, "nearestDistance", np.float32(0.125))]
    for q in range(1, 13):
        expect += [(q, "count", 0), (q, "firstRow", -1), (q, "bestRow", -1), (q, "nearestRow", p)]
    differs = [(q, "count") for q in range(1, 13)] + [(q, "nearestRow") for q in range(1, 13)]
    return state, ctrl, goals, mask, expect, differs


def masked_row_plants(R: int):
    """The rows masked_rows(R) plants, ascending, and whether each is alive: the plants of
    single(R), and in the long trees the rows round the ends of the sweeps; alive and dead by
    turns, the last row alive."""
    rows = sorted({p for p in (0, 63, 64, 255, 256, SWEEP - 1, SWEEP, SWEEP + 40, 2 * SWEEP - 1, 2 * SWEEP, R - 2,
                               R - 1) if 0 <= p < R})
    return rows, [(len(rows) - 1 - k) % 2 == 0 for k in range(len(rows))]


def masked_rows(R: int):
    """One planted row per goal, alive and dead by turns, and a pseudo-random third of the
    background dead.  A goal whose planted row is dead has nothing inside, and its nearest row is
    the nearest alive planted row of another goal: in the long trees a row of a later sweep."""
    state, ctrl = background(R)
    mask = (np.random.default_rng(R).integers(0, 3, size=R) != 0).astype(np.uint8)
    rows, alive = masked_row_plants(R)
    goals, expect, differs = [], [], []
    for k, (p, a) in enumerate(zip(rows, alive)):
        cx, cy = 10.0 + 8.0 * (k % 6), 10.0 + 8.0 * (k // 6)
        _plant(state, ctrl, p, cx + 0.125, cy, 3.0 + k)
        mask[p] = 1 if a else 0
        goals.append((cx, cy, 0.5))
        if a:
            expect += [(k, "count", 1), (k, "firstRow", p), (k, "bestRow", p), (k, "nearestRow", p),
                       (k, "bestCost", np.float32(3.0 + k)), (k, "nearestDistance", np.float32(0.125))]
        else:
            expect += [(k, "count", 0), (k, "firstRow", -1), (k, "bestRow", -1), (k, "bestCost", np.float32(0.0))]
            differs += [(k, "count"), (k, "nearestRow")]
    return state, ctrl, goals, mask, expect, differs


def masked_goals(Q: int):
    """The scattered rows and goals of goal_count(Q) with half the rows dead."""
    state, ctrl, goals, _ = goal_count(Q)
    return state, ctrl, goals, _scattered_mask(len(state), 200 + Q), [], [(q, "count") for q in range(Q)]


def masked_nonfinite():
    """_NONFINITE: a row with x = NaN, one with y = +inf and an inside row of cost +inf, each once
    alive and once dead.  Every goal keeps alive finite rows, so no answer holds a NaN."""
    state, ctrl, goals, mask = _nonfinite_rows()
    expect = [(0, "count", 2), (0, "firstRow", 10), (0, "bestRow", 10), (0, "bestCost", np.float32(3.0)),
              (0, "nearestRow", 300), (0, "nearestDistance", np.float32(0.125)),
              (1, "count", 1), (1, "bestRow", 400), (1, "bestCost", np.float32(np.inf)), (1, "nearestRow", 400),
              (2, "count", int(mask.sum()) - 2), (2, "firstRow", 0), (2, "nearestRow", 300),
              (3, "count", 0)]
    differs = [(0, "count"), (0, "nearestRow"), (1, "count"), (1, "bestRow"), (1, "bestCost"), (2, "count")]
    return state, ctrl, goals, mask, expect, differs


MASKED_BUILDERS = {"masked-ties": masked_ties, "masked-radius-edges": masked_radius_edges,
                   "masked-zero-distance": masked_zero_distance, "masked-bytes": masked_bytes,
                   "masked-bytes-01": masked_bytes_01, "masked-none": masked_none}
MASKED_BUILDERS.update({f"masked-one-{p}": functools.partial(masked_one, p) for p in ONE_ROWS})
MASKED_BUILDERS.update({f"masked-rows-{R}": functools.partial(masked_rows, R) for R in MASKED_ROW_COUNTS})
MASKED_BUILDERS.update({f"masked-goals-{Q}": functools.partial(masked_goals, Q) for Q in MASKED_GOAL_COUNTS})
MASKED_BUILDERS["masked-nonfinite"] = masked_nonfinite
MASKED_NAMES = tuple(MASKED_BUILDERS)


@functools.lru_cache(maxsize=None)
def masked_case(name: str) -> MaskedCase:
    """Built and modelled once, read-only; the preconditions in `differs` hold or this raises."""
    state, ctrl, goals, mask, expect, differs = MASKED_BUILDERS[name]()
    goals = np.asarray(goals, dtype=np.float32).reshape(-1, 3)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    assert mask.shape == (len(state),)
    model, unmasked = model_of_rows(state, ctrl, goals, mask), model_of_rows(state, ctrl, goals)
    # a one-row tree with its row alive is the one mask that cannot matter
    assert differs or (len(state) == 1 and mask.all()), f"{name}: a masked case says where its mask matters"
    for q, field in differs:
        a, b = np.asarray(model[field][q:q + 1]), np.asarray(unmasked[field][q:q + 1])
        assert a.tobytes() != b.tobytes(), f"{name}: the mask changes nothing in {field} of goal {q}"
    for a in (state, ctrl, goals, mask, *model.values(), *unmasked.values()):
        a.setflags(write=False)
    return MaskedCase(name, state, ctrl, goals, mask, tuple(expect), tuple(differs), model, unmasked)

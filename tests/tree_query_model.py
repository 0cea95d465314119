"""The goal query over tree rows as a numpy float32 model (no GPU, no library).

For a row (x, y, cost) and a goal (gx, gy, r), each operation a separate float32 ufunc
call (so none is fused):

    dx = x - gx,  dy = y - gy,  d2 = dx * dx + dy * dy
    the row is inside  iff  sqrt(d2) < r          (np.sqrt is correctly rounded)

and per goal, over the rows [0, R):

    count                         rows inside
    firstRow                      the lowest row inside, -1 if none
    bestRow, bestCost             the inside row of lowest cost, lowest row on ties (the
                                  lexicographic minimum of (cost bits, row)); -1 and 0 if none
    nearestRow, nearestDistance   the lexicographic minimum of (d2 bits, row): the lowest d2, the
                                  lowest row on ties, a NaN d2 above +inf by its bit pattern as
                                  include/sbmp/tree_query.h orders it (nearest_of; np.argmin,
                                  which agrees wherever no d2 is NaN, takes a NaN for the
                                  minimum); and sqrt of that d2

With a mask (model_of_rows(..., alive)): a row is skipped iff its byte is 0, the rows that
remain answer as above under the tree's own row numbers, and with none left the answer is
count 0, firstRow -1, bestRow -1, bestCost 0, nearestRow -1, nearestDistance +inf.

Written from the definition; it shares no code with the library.  numpy over KGMT.tree()
is what KGMT.query_goals must return: tree_rows() cuts the export to the rows it scans.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("count", "firstRow", "bestRow", "bestCost", "nearestRow", "nearestDistance")


def d2_of(x: np.ndarray, y: np.ndarray, gx, gy) -> np.ndarray:
    gx, gy = np.float32(gx), np.float32(gy)
    with np.errstate(all="ignore"):
        dx = np.subtract(x, gx, dtype=np.float32)
        dy = np.subtract(y, gy, dtype=np.float32)
        xx = np.multiply(dx, dx, dtype=np.float32)
        yy = np.multiply(dy, dy, dtype=np.float32)
        return np.add(xx, yy, dtype=np.float32)


def inside_of(d2: np.ndarray, r) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.less(np.sqrt(d2, dtype=np.float32), np.float32(r))


def nearest_of(d2: np.ndarray) -> int:
    """The row of the lowest (d2 bits, row)."""
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(d2), dtype=np.uint64)
    return int(np.argmin(key))


def empty_answers(Q: int) -> dict:
    """The answer over no rows at all, Q times."""
    return {"count": np.zeros(Q, np.int32), "firstRow": np.full(Q, -1, np.int32), "bestRow": np.full(Q, -1, np.int32),
            "bestCost": np.zeros(Q, np.float32), "nearestRow": np.full(Q, -1, np.int32),
            "nearestDistance": np.full(Q, np.inf, np.float32)}


def query_model(x, y, cost, goals) -> dict:
    """x, y, cost: (R,) float32; goals: (Q, 3) rows of (gx, gy, r).  A dict of (Q,) arrays."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    goals = np.asarray(goals, dtype=np.float32).reshape(-1, 3)
    Q = len(goals)
    out = {"count": np.zeros(Q, np.int32), "firstRow": np.full(Q, -1, np.int32), "bestRow": np.full(Q, -1, np.int32),
           "bestCost": np.zeros(Q, np.float32), "nearestRow": np.zeros(Q, np.int32),
           "nearestDistance": np.zeros(Q, np.float32)}
    for q, (gx, gy, r) in enumerate(goals):
        d2 = d2_of(x, y, gx, gy)
        rows = np.flatnonzero(inside_of(d2, r))
        out["count"][q] = len(rows)
        if len(rows):
            out["firstRow"][q] = rows[0]
            order = np.lexsort((rows, cost[rows].view(np.uint32)))   # by cost bits, then by row
            out["bestRow"][q] = rows[order[0]]
            out["bestCost"][q] = cost[rows[order[0]]]
        k = nearest_of(d2)
        out["nearestRow"][q] = k
        with np.errstate(all="ignore"):
            out["nearestDistance"][q] = np.sqrt(d2[k], dtype=np.float32)
    return out


def tree_rows(samples, costs, tree_size):
    """(state (R, 4), ctrl (R, 4)) of the rows a query scans, R = min(treeSize, M), from the
    export layout of KGMT.tree(): samples (M, 7), costs (M,)."""
    R = min(int(tree_size), len(costs))
    state = np.ascontiguousarray(samples[:R, :4], dtype=np.float32)
    ctrl = np.ascontiguousarray(np.concatenate([samples[:R, 4:7], costs[:R, None]], axis=1), dtype=np.float32)
    return state, ctrl


def model_of_rows(state, ctrl, goals, alive=None) -> dict:
    """The model over the rows, or over np.flatnonzero(alive) with the row numbers mapped back."""
    if alive is None:
        return query_model(state[:, 0], state[:, 1], ctrl[:, 3], goals)
    idx = np.flatnonzero(np.asarray(alive).reshape(-1))
    assert len(np.asarray(alive).reshape(-1)) == len(state)
    if len(idx) == 0:
        return empty_answers(len(np.asarray(goals, dtype=np.float32).reshape(-1, 3)))
    m = query_model(state[idx, 0], state[idx, 1], ctrl[idx, 3], goals)
    for k in ("firstRow", "bestRow", "nearestRow"):
        m[k] = np.where(m[k] >= 0, idx[np.maximum(m[k], 0)], -1).astype(np.int32)
    return m


def assert_same_answers(got: dict, want: dict, label: str = "") -> None:
    """Bit-exact on every field (floats through their bit patterns)."""
    for k in FIELDS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, f"{label} {k}: {g.shape} vs {w.shape}"
        if w.dtype == np.float32:
            g, w = g.astype(np.float32).view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{label} {k}: goals {bad[:8].tolist()} got {got[k][bad[:8]]} want {want[k][bad[:8]]}"

"""Goal queries against tree rows (include/sbmp/tree_query.h) over numpy arrays.

    goal_radius_threshold  t(r): the largest float d2 with sqrtf(d2) < r (host-only)
    tree_query_batch       k_tree_query over caller rows on the GPU (sbmp_tree_query_batch), or,
                           with device=False, the host loop that applies the literal
                           sqrtf(d2) < r rule to every row (sbmp_tree_query_batch_host); with a
                           mask, k_tree_query_alive (sbmp_tree_query_alive_batch) and its host loop

KGMT.query_goals (cudasbmp_amd.kgmt) asks the same of a planner's own tree.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat

ANSWER_FIELDS = tuple(n for n, _ in nat.GoalAnswer._fields_)
ANSWER_DTYPE = np.dtype(nat.GoalAnswer)


def goal_radius_threshold(r: float) -> np.float32:
    t = ctypes.c_float()
    nat.call("sbmp_goal_radius_threshold", ctypes.c_float(r), ctypes.byref(t))
    return np.float32(t.value)


def goal_array(goals, radius=None) -> np.ndarray:
    """(Q, 3) float32 rows (x, y, radius) from (Q, 2) goals and one radius, or from (Q, 3) goals."""
    g = np.asarray(goals, dtype=np.float32)
    g = g.reshape(-1, g.shape[-1]) if g.ndim else g.reshape(0, 3)
    if radius is None:
        if g.shape[1] != 3:
            raise ValueError("goals must be (Q, 3) rows of (x, y, radius) when no radius is given")
    else:
        if g.shape[1] != 2:
            raise ValueError("goals must be (Q, 2) rows of (x, y) when a radius is given")
        g = np.concatenate([g, np.full((len(g), 1), radius, dtype=np.float32)], axis=1)
    return np.ascontiguousarray(g, dtype=np.float32)


def answers_dict(out: np.ndarray) -> dict:
    """The answer records as one numpy array per field of sbmp_goal_answer."""
    return {k: out[k].copy() for k in ANSWER_FIELDS}


def tree_query_batch(state, ctrl, goals, radius=None, *, alive=None, device=True) -> dict:
    """state (R, 4) float32 rows (x, y, -, -), ctrl (R, 4) float32 rows (-, -, -, cost): the
    planner's tree layout.  alive: (R,) uint8, passed on as it is (any other type: != 0); a row
    whose byte is 0 is skipped, and the masked kernel answers.  Returns a dict of (Q,) arrays:
    count, firstRow, bestRow, bestCost, nearestRow, nearestDistance."""
    from .batch import _Dev
    st = np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4)
    ct = np.ascontiguousarray(ctrl, dtype=np.float32).reshape(-1, 4)
    if len(st) != len(ct):
        raise ValueError("state and ctrl must have the same number of rows")
    mask = None
    if alive is not None:
        mask = np.asarray(alive)
        mask = np.ascontiguousarray(mask if mask.dtype == np.uint8 else mask != 0, dtype=np.uint8).reshape(-1)
        if len(mask) != len(st):
            raise ValueError("alive must have one byte per row")
    g = goal_array(goals, radius)
    out = np.zeros(max(1, len(g)), dtype=ANSWER_DTYPE)
    gp, op = g.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    if not device:
        if mask is None:
            nat.call("sbmp_tree_query_batch_host", hp(st), hp(ct), len(st), gp, len(g), op)
        else:
            nat.call("sbmp_tree_query_alive_batch_host", hp(st), hp(ct), hp(mask), len(st), gp, len(g), op)
        return answers_dict(out[: len(g)])
    devs = []
    try:
        for a in (st, ct) + (() if mask is None else (mask,)):
            devs.append(_Dev(a))
        dp = [ctypes.c_void_p(d.ptr) for d in devs]
        if mask is None:
            nat.call("sbmp_tree_query_batch", dp[0], dp[1], len(st), gp, len(g), op, None)
        else:
            nat.call("sbmp_tree_query_alive_batch", dp[0], dp[1], dp[2], len(st), gp, len(g), op, None)
    finally:
        for d in devs:
            d.close()
    return answers_dict(out[: len(g)])

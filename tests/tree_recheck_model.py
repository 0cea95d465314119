"""The tree re-check as a model that shares no code with the library (include/sbmp/tree_recheck.h
states the rule): oracle.pyoracle.replay, the CPU oracle's own re-propagation of parents and
stored controls, gives every row's replayed state and verdict; numpy applies the orphan rule
and the bit comparison, and a plain ascending loop decides `alive`.

    FREE 0      row 0; r > 0: the replay stays valid and ends on the stored state bit for bit
    ORPHAN 1    r > 0 and parent not in [0, r): nothing is replayed through it (the model
                replays row 0 in its place and throws the result away)
    BLOCKED 2   the replay ends invalid
    STALE 3     valid, but not the stored state
    alive[r] = status[r] == FREE and (r == 0 or alive[parent[r]]);  exported byte | CUT (0x80)
    for a FREE row that is not alive
"""
from __future__ import annotations

import numpy as np

FREE, ORPHAN, BLOCKED, STALE, CUT = 0, 1, 2, 3, 0x80
SUMMARY = ("rows", "alive", "blocked", "stale", "orphan", "cut", "firstDead")


def planner_config(numDisc=10, agentLength=1.0, width=20.0, height=20.0, agent="car"):
    from oracle.pyoracle import PlannerConfig
    return PlannerConfig(width=width, height=height, numDisc=numDisc, agentLength=agentLength,
                         agent=1 if agent == "point" else 0)


def replay_rows(state, ctrl, parent, obstacles, *, threads=8, **params):
    """(usable, replayed (R, 4), valid (R,)) of every row; rows without a usable parent replay row 0."""
    from oracle.pyoracle import replay
    state = np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4)
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float32).reshape(-1, 4)
    parent = np.ascontiguousarray(parent, dtype=np.int32).ravel()
    R = len(state)
    idx = np.arange(R, dtype=np.int64)
    usable = (parent >= 0) & (parent.astype(np.int64) < idx)
    par = np.where(usable, parent, 0)
    boxes = np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 4)
    out, valid = replay(planner_config(**params), boxes, state[par], np.ascontiguousarray(ctrl[:, :3]), threads=threads)
    return usable, out, valid


def recheck_model(state, ctrl, parent, obstacles, *, threads=8, **params):
    """(exported status (R,) uint8, summary dict, alive (R,) bool)."""
    state = np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4)
    parent = np.ascontiguousarray(parent, dtype=np.int32).ravel()
    R = len(state)
    usable, out, valid = replay_rows(state, ctrl, parent, obstacles, threads=threads, **params)
    same = (out.view(np.uint32) == state.view(np.uint32)).all(axis=1)
    status = np.full(R, STALE, np.uint8)
    status[valid & same] = FREE
    status[~valid] = BLOCKED
    status[~usable] = ORPHAN
    status[0] = FREE
    alive = np.zeros(R, bool)
    free = (status == FREE).tolist()
    par = parent.tolist()
    live = [False] * R
    for r in range(R):                       # ascending: a usable parent is a lower row
        live[r] = free[r] and (r == 0 or live[par[r]])
    alive[:] = live
    exported = status.copy()
    exported[(status == FREE) & ~alive] = FREE | CUT
    return exported, summary_of(exported), alive


def summary_of(exported) -> dict:
    e = np.asarray(exported, np.uint8)
    dead = np.flatnonzero(e != FREE)
    return {"rows": len(e), "alive": int((e == FREE).sum()), "blocked": int((e == BLOCKED).sum()),
            "stale": int((e == STALE).sum()), "orphan": int((e == ORPHAN).sum()), "cut": int((e == (FREE | CUT)).sum()),
            "firstDead": int(dead[0]) if len(dead) else -1}


def tree_arrays(samples, parent, costs, tree_size):
    """(state (R, 4), ctrl (R, 4), parent (R,)) of the rows a re-check covers, R = min(treeSize, M)
    (at least 1), from the export layout of KGMT.tree() / Oracle.tree()."""
    R = max(1, min(int(tree_size), len(parent)))
    state = np.ascontiguousarray(samples[:R, :4], dtype=np.float32)
    ctrl = np.ascontiguousarray(np.concatenate([samples[:R, 4:7], costs[:R, None]], axis=1), dtype=np.float32)
    return state, ctrl, np.ascontiguousarray(parent[:R], dtype=np.int32)


def depths(parent) -> np.ndarray:
    """Edges between each row and the root along usable parents (an orphan counts as a root)."""
    p = np.asarray(parent).tolist()
    d = [0] * len(p)
    for r in range(1, len(p)):
        d[r] = d[p[r]] + 1 if 0 <= p[r] < r else 0
    return np.array(d, np.int64)


def descendants(parent) -> np.ndarray:
    """Rows strictly below each row."""
    p = np.asarray(parent).tolist()
    n = [0] * len(p)
    for r in range(len(p) - 1, 0, -1):
        if 0 <= p[r] < r:
            n[p[r]] += n[r] + 1
    return np.array(n, np.int64)


def assert_same_recheck(got, want, label=""):
    """(status, summary) pairs, byte for byte and field for field."""
    gs, gm = got
    ws, wm = want
    gs, ws = np.asarray(gs, np.uint8), np.asarray(ws, np.uint8)
    assert gs.shape == ws.shape, f"{label}: {gs.shape} vs {ws.shape}"
    bad = np.flatnonzero(gs != ws)
    assert len(bad) == 0, f"{label}: {len(bad)} rows differ, first {bad[:8].tolist()}: got {gs[bad[:8]]} want {ws[bad[:8]]}"
    assert {k: gm[k] for k in SUMMARY} == {k: wm[k] for k in SUMMARY}, f"{label}: summary {gm} vs {wm}"
    assert gm["rows"] == gm["alive"] + gm["blocked"] + gm["stale"] + gm["orphan"] + gm["cut"]

"""Re-anchoring as a model that shares no code with the library (include/sbmp/tree_reanchor.h
states the rule): tests/tree_recheck_model.py's `depths` gives every row's level; level by level
oracle.pyoracle.replay, the CPU oracle's own propagation, runs the rows whose parent is alive
from the parents' NEW states with the rows' stored controls; numpy applies the orphan and cut
rules.

    row 0                  FREE, alive, out[0] = s0
    parent not in [0, r)   ORPHAN 1, dead
    parent dead            FREE | CUT 0x80, dead, not replayed
    parent alive           the replay valid: FREE 0, alive, out[r] = its end state; else BLOCKED 2, dead
    out[r] = state[r] bit for bit for every dead row
    levels = 1 + the deepest row's edges to the top of its chain
"""
from __future__ import annotations

import numpy as np

from tree_recheck_model import BLOCKED, CUT, FREE, ORPHAN, depths, planner_config

SUMMARY = ("rows", "alive", "blocked", "orphan", "cut", "firstDead", "levels")


def reanchor_model(state, ctrl, parent, s0, obstacles, *, threads=8, **params):
    """(out (R, 4) float32, alive (R,) bool, status (R,) uint8, summary dict)."""
    from oracle.pyoracle import replay
    state = np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4)
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float32).reshape(-1, 4)
    parent = np.ascontiguousarray(parent, dtype=np.int32).ravel()
    boxes = np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 4)
    cfg = planner_config(**params)
    R = len(state)
    d = depths(parent)
    out = state.copy()
    out[0] = np.asarray(s0, np.float32)[:4]
    alive = np.zeros(R, bool)
    alive[0] = True
    status = np.full(R, ORPHAN, np.uint8)       # what a depth-0 row other than row 0 is
    status[0] = FREE
    order = np.argsort(d, kind="stable")
    bounds = np.searchsorted(d[order], np.arange(int(d.max()) + 2))
    for lv in range(1, int(d.max()) + 1):
        rows = order[bounds[lv]:bounds[lv + 1]]
        live = alive[parent[rows]]
        status[rows[~live]] = FREE | CUT
        run = rows[live]
        if len(run) == 0:
            continue
        end, valid = replay(cfg, boxes, np.ascontiguousarray(out[parent[run]]), np.ascontiguousarray(ctrl[run, :3]),
                            threads=threads)
        valid = np.asarray(valid, bool)
        ok = run[valid]
        out[ok] = end[valid]
        alive[ok] = True
        status[ok] = FREE
        status[run[~valid]] = BLOCKED
    return out, alive, status, summary_of(status, int(d.max()) + 1)


def summary_of(status, levels) -> dict:
    e = np.asarray(status, np.uint8)
    dead = np.flatnonzero(e != FREE)
    return {"rows": len(e), "alive": int((e == FREE).sum()), "blocked": int((e == BLOCKED).sum()),
            "orphan": int((e == ORPHAN).sum()), "cut": int((e == (FREE | CUT)).sum()),
            "firstDead": int(dead[0]) if len(dead) else -1, "levels": int(levels)}


def assert_same_reanchor(got, want, label=""):
    """got: the dict tree_reanchor_batch returns; want: reanchor_model's tuple.  Bit for bit."""
    wout, walive, wstatus, wsum = want
    gs = np.asarray(got["status"], np.uint8)
    assert gs.shape == wstatus.shape, f"{label}: {gs.shape} vs {wstatus.shape}"
    bad = np.flatnonzero(gs != wstatus)
    assert len(bad) == 0, (f"{label}: {len(bad)} status bytes differ, first {bad[:8].tolist()}: got {gs[bad[:8]]} "
                           f"want {wstatus[bad[:8]]}")
    assert np.array_equal(np.asarray(got["alive"], np.uint8), walive.astype(np.uint8)), f"{label}: alive"
    g = np.ascontiguousarray(got["state"], np.float32).view(np.uint32)
    bad = np.flatnonzero((g != wout.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (f"{label}: {len(bad)} states differ, first {bad[:4].tolist()}: got "
                           f"{got['state'][bad[:2]].tolist()} want {wout[bad[:2]].tolist()}")
    gm = got["summary"]
    assert {k: gm[k] for k in SUMMARY} == wsum, f"{label}: summary {gm} vs {wsum}"
    assert gm["rows"] == gm["alive"] + gm["blocked"] + gm["orphan"] + gm["cut"]

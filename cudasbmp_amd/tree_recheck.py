"""The tree re-check (include/sbmp/tree_recheck.h) over numpy arrays.

    tree_recheck_batch   k_tree_recheck + k_tree_alive over caller rows on the GPU
                         (sbmp_tree_recheck_batch), or, with device=False, the host loop that
                         applies the literal rule row by row (sbmp_tree_recheck_batch_host)

KGMT.recheck (cudasbmp_amd.kgmt) asks the same of a planner's own tree.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat

FREE, ORPHAN, BLOCKED, STALE, CUT = (nat.SBMP_ROW_FREE, nat.SBMP_ROW_ORPHAN, nat.SBMP_ROW_BLOCKED,
                                     nat.SBMP_ROW_STALE, nat.SBMP_ROW_CUT)
SUMMARY_FIELDS = tuple(n for n, _ in nat.TreeRecheck._fields_)


def tree_recheck_batch(state, ctrl, parent, obstacles, *, numDisc=10, agentLength=1.0, width=20.0, height=20.0,
                       agent="car", depthBound=0, device=True):
    """state (R, 4) float32 rows (x, y, theta, v), ctrl (R, 4) float32 rows (a, steering, duration, -),
    parent (R,) int32: the planner's tree layout; obstacles (n, 4).  depthBound: an upper bound on
    the rows of any parent chain, 0 for R.  Returns (status (R,) uint8, summary dict)."""
    from .batch import _Dev
    host = {"state": np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4),
            "ctrl": np.ascontiguousarray(ctrl, dtype=np.float32).reshape(-1, 4),
            "parent": np.ascontiguousarray(parent, dtype=np.int32).ravel(),
            "obstacles": np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 4)}
    R = len(host["state"])
    if len(host["ctrl"]) != R or len(host["parent"]) != R:
        raise ValueError("state, ctrl and parent must have the same number of rows")
    a = nat.TreeRecheckArgs()
    a.rows, a.depthBound, a.obstaclesCount = R, int(depthBound), len(host["obstacles"])
    a.agent = nat.SBMP_AGENT_POINT if agent == "point" else nat.SBMP_AGENT_CAR
    a.numDisc, a.agentLength, a.width, a.height = numDisc, agentLength, width, height
    status = np.zeros(max(1, R), dtype=np.uint8)
    s = nat.TreeRecheck()
    devs = {}
    try:
        for name, arr in host.items():
            if name == "obstacles" and not len(arr):
                continue   # a NULL list with count 0
            if device:
                devs[name] = _Dev(arr)
                setattr(a, name, devs[name].ptr)
            else:
                setattr(a, name, arr.ctypes.data)
        if device:
            nat.call("sbmp_tree_recheck_batch", ctypes.byref(a), status.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s),
                     None)
        else:
            nat.call("sbmp_tree_recheck_batch_host", ctypes.byref(a), status.ctypes.data_as(ctypes.c_void_p),
                     ctypes.byref(s))
    finally:
        for d in devs.values():
            d.close()
    return status[:R], {k: getattr(s, k) for k in SUMMARY_FIELDS}

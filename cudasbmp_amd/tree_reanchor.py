"""A grown tree re-anchored on a measured root state (include/sbmp/tree_reanchor.h).

    tree_reanchor_batch   the k_reanchor_* kernels over caller rows on the GPU, one launch per
                          level of the tree (sbmp_tree_reanchor_batch), or, with device=False, the
                          host loop that applies the literal rule row by row
                          (sbmp_tree_reanchor_batch_host)
    reanchor, replan_from what KGMT.reanchor and KGMT.replan_from (cudasbmp_amd.kgmt) call
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat

SUMMARY_FIELDS = tuple(n for n, _ in nat.TreeReanchor._fields_)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _summary(s) -> dict:
    return {k: getattr(s, k) for k in SUMMARY_FIELDS}


def _root4(new_root) -> np.ndarray:
    r = np.ascontiguousarray(new_root, dtype=np.float32).ravel()
    if len(r) < 4:
        raise ValueError("new_root must be (x, y, theta, v)")
    return r[:4].copy()


def tree_reanchor_batch(state, ctrl, parent, new_root, obstacles, *, device=True, depth_bound=0, numDisc=10,
                        agentLength=1.0, width=20.0, height=20.0, agent="car") -> dict:
    """state (R, 4) float32 rows (x, y, theta, v), ctrl (R, 4) float32 rows (a, steering, duration,
    cost), parent (R,) int32: the planner's tree layout, root = row 0; new_root (x, y, theta, v);
    obstacles (n, 4).  depth_bound: an upper bound on the rows of any parent chain, 0 for R; one
    that is too small is refused.  Returns state (R, 4), the new states (a dead row keeps its
    stored one), alive (R,) uint8, status (R,) uint8 (SBMP_ROW_*) and summary, a dict rows, alive,
    blocked, orphan, cut, firstDead, levels."""
    from .batch import _Dev
    host = {"state": np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4),
            "ctrl": np.ascontiguousarray(ctrl, dtype=np.float32).reshape(-1, 4),
            "parent": np.ascontiguousarray(parent, dtype=np.int32).ravel(),
            "obstacles": np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 4)}
    R = len(host["state"])
    if len(host["ctrl"]) != R or len(host["parent"]) != R:
        raise ValueError("state, ctrl and parent must have the same number of rows")
    s0 = _root4(new_root)
    a = nat.TreeRecheckArgs()
    a.rows, a.depthBound, a.obstaclesCount = R, int(depth_bound), len(host["obstacles"])
    a.agent = nat.SBMP_AGENT_POINT if agent == "point" else nat.SBMP_AGENT_CAR
    a.numDisc, a.agentLength, a.width, a.height = numDisc, agentLength, width, height
    out_state = np.zeros((max(1, R), 4), dtype=np.float32)
    alive = np.zeros(max(1, R), dtype=np.uint8)
    status = np.zeros(max(1, R), dtype=np.uint8)
    s = nat.TreeReanchor()
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
            devs["out"], devs["alive"] = _Dev(out_state), _Dev(alive)
            nat.call("sbmp_tree_reanchor_batch", ctypes.byref(a), _vp(s0), ctypes.c_void_p(devs["out"].ptr),
                     ctypes.c_void_p(devs["alive"].ptr), _vp(status), ctypes.byref(s), None)
            out_state, alive = devs["out"].get(), devs["alive"].get()
        else:
            nat.call("sbmp_tree_reanchor_batch_host", ctypes.byref(a), _vp(s0), _vp(out_state), _vp(alive), _vp(status),
                     ctypes.byref(s))
    finally:
        for d in devs.values():
            d.close()
    return {"state": out_state[:R], "alive": alive[:R], "status": status[:R], "summary": _summary(s)}


def reanchor(kgmt, new_root, root, obstacles, obstaclesCount=None) -> dict:
    """KGMT.reanchor: obstacles is an (n, 4) array, or a device pointer with obstaclesCount."""
    from .kgmt import DeviceBuffer, device_ptr
    s0 = _root4(new_root)
    s = nat.TreeReanchor()
    own = None
    try:
        if obstaclesCount is None:
            boxes = np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 4)
            obstaclesCount = len(boxes)
            own = DeviceBuffer(boxes) if obstaclesCount else None
            ptr = own.ptr if own is not None else None
        else:
            ptr = device_ptr(obstacles) if obstaclesCount else None

        def call(state, ctrl, parent, origin, status, capacity):
            nat.call("sbmp_kgmt_reanchor_tree", kgmt._h, int(root), _vp(s0), ctypes.c_void_p(ptr), int(obstaclesCount),
                     state, ctrl, parent, origin, status, capacity, ctypes.byref(s))

        ex = nat.TreeExtract()   # the size: the extraction keeps every row below the root
        nat.call("sbmp_kgmt_extract_tree", kgmt._h, int(root), 0, None, None, None, None, None, 0, ctypes.byref(ex))
        cap = max(1, ex.kept)
        out = {"state": np.zeros((cap, 4), dtype=np.float32), "ctrl": np.zeros((cap, 4), dtype=np.float32),
               "parent": np.zeros(cap, dtype=np.int32), "origin": np.zeros(cap, dtype=np.int32),
               "status": np.zeros(cap, dtype=np.uint8)}
        call(*(_vp(out[k]) for k in ("state", "ctrl", "parent", "origin", "status")), cap)
    finally:
        if own is not None:
            own.free()
    out = {k: v[: s.rows].copy() for k, v in out.items()}
    out["alive"] = (out["status"] == nat.SBMP_ROW_FREE).astype(np.uint8)
    out["summary"] = _summary(s)
    return out


def replan_from(kgmt, new_root, goal, d_obstacles, count, seed, root=0, frontier_from=0) -> dict:
    from .kgmt import _vec7, device_ptr
    from .tree_adopt import SUMMARY_FIELDS as ADOPT_FIELDS
    s0 = _root4(new_root)
    g = _vec7(goal)
    ra, ad = nat.TreeReanchor(), nat.TreeAdopt()
    kgmt._obs_keepalive = d_obstacles
    nat.call("sbmp_kgmt_replan_from", kgmt._h, int(root), _vp(s0), int(frontier_from), _vp(g),
             ctypes.c_void_p(device_ptr(d_obstacles)), int(count), int(seed), ctypes.byref(ra), ctypes.byref(ad))
    return {"reanchor": _summary(ra), "adopt": {k: getattr(ad, k) for k in ADOPT_FIELDS}}

"""A tree adopted into a planner as its iteration 1 (include/sbmp/tree_adopt.h).

    tree_adopt_tables   the tables an adoption leaves, over caller rows and any grid: the
                        k_adopt_* kernels on the GPU (sbmp_tree_adopt_tables), or, with
                        device=False, the host loop that applies the literal rule
                        (sbmp_tree_adopt_tables_host)
    adopt, replan       what KGMT.adopt and KGMT.replan (cudasbmp_amd.kgmt) call
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat

SUMMARY_FIELDS = tuple(k for k, _ in nat.TreeAdopt._fields_)
R1_TABLES = ("R1", "R1Avail", "R1Valid", "R1Invalid", "R1Cov")


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _summary(s) -> dict:
    return {k: getattr(s, k) for k in SUMMARY_FIELDS}


def tree_adopt_tables(state, *, width=20.0, height=20.0, N=16, n=8, goal=None, frontier_from=0, device=True,
                      stream=None) -> dict:
    """state (R, 4) rows of (x, y, theta, v); the grid (width, height, N, n); goal: (x, y, radius)
    or None for no disc.  Returns the five R1 tables (N * N,) int32, R2bits (ceil(N N n n / 32),)
    uint32 with bit r2 & 31 of word r2 >> 5, and summary, a dict rows, nonFinite,
    frontierNonFinite, outOfGrid, goalRow, treeSize, gLo."""
    from .batch import _Dev
    st = np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4)
    R = len(st)
    a = nat.TreeAdoptTablesArgs()
    a.rows, a.frontierFrom = R, int(frontier_from)
    a.width, a.height, a.N, a.n = float(width), float(height), int(N), int(n)
    g = None if goal is None else np.ascontiguousarray(goal, dtype=np.float32).ravel()[:3].copy()
    if g is not None and len(g) != 3:
        raise ValueError("goal must be (x, y, radius)")
    a.goal = g.ctypes.data if g is not None else None
    nR1 = max(1, int(N) * int(N))
    nW = max(1, (nR1 * int(n) * int(n) + 31) // 32)
    out = {k: np.zeros(nR1, dtype=np.int32) for k in R1_TABLES}
    out["R2bits"] = np.zeros(nW, dtype=np.uint32)
    s = nat.TreeAdopt()
    ptrs = [_vp(out[k]) for k in R1_TABLES + ("R2bits",)]
    dev = None
    try:
        if device:
            if R:
                dev = _Dev(st)
                a.state = dev.ptr
            nat.call("sbmp_tree_adopt_tables", ctypes.byref(a), *ptrs, ctypes.byref(s), ctypes.c_void_p(stream or 0))
        else:
            a.state = st.ctypes.data if R else None
            nat.call("sbmp_tree_adopt_tables_host", ctypes.byref(a), *ptrs, ctypes.byref(s))
    finally:
        if dev is not None:
            dev.close()
    out["summary"] = _summary(s)
    return out


def adopt(kgmt, samples, parents, costs, goal, d_obstacles, count, seed, frontier_from=0, depth_bound=0) -> dict:
    """KGMT.adopt: samples (R, 7), parents (R,), costs (R,) as KGMT.tree() returns them (or state
    (R, 4) and ctrl (R, 4) as KGMT.extract() does: pass samples=state, costs=ctrl)."""
    from .kgmt import _vec7, device_ptr
    s = np.ascontiguousarray(samples, dtype=np.float32)
    c = np.ascontiguousarray(costs, dtype=np.float32)
    p = np.ascontiguousarray(parents, dtype=np.int32).ravel()
    if s.ndim == 2 and s.shape[1] == 7:
        state = np.ascontiguousarray(s[:, :4])
        ctrl = np.ascontiguousarray(np.concatenate([s[:, 4:7], c.reshape(-1, 1)], axis=1))
    else:
        state, ctrl = s.reshape(-1, 4), c.reshape(-1, 4)
    if not (len(state) == len(ctrl) == len(p)):
        raise ValueError("samples, parents and costs must have one row per tree row")
    a = nat.TreeAdoptArgs()
    a.state, a.ctrl, a.parent = state.ctypes.data, ctrl.ctypes.data, p.ctypes.data
    a.rows, a.frontierFrom, a.depthBound, a.onDevice = len(p), int(frontier_from), int(depth_bound), 0
    g = _vec7(goal)
    out = nat.TreeAdopt()
    kgmt._obs_keepalive = d_obstacles
    nat.call("sbmp_kgmt_adopt_tree", kgmt._h, ctypes.byref(a), _vp(g), ctypes.c_void_p(device_ptr(d_obstacles)),
             int(count), int(seed), ctypes.byref(out))
    return _summary(out)


def replan(kgmt, goal, d_obstacles, count, seed, root=0, alive=False, frontier_from=0) -> dict:
    from .kgmt import _vec7, device_ptr
    g = _vec7(goal)
    out = nat.TreeAdopt()
    kgmt._obs_keepalive = d_obstacles
    nat.call("sbmp_kgmt_replan", kgmt._h, int(root), int(bool(alive)), int(frontier_from), _vp(g),
             ctypes.c_void_p(device_ptr(d_obstacles)), int(count), int(seed), ctypes.byref(out))
    return _summary(out)

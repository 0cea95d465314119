"""Paths and traces of a grown tree (include/sbmp/tree_paths.h) over numpy arrays.

    tree_paths_batch   k_path_walk over caller rows on the GPU (sbmp_tree_paths_batch), or, with
                       device=False, the host loop that applies the literal rule
                       (sbmp_tree_paths_batch_host)
    tree_trace_batch   k_tree_trace likewise (sbmp_tree_trace_batch / _host); the tree and the row
                       list may be torch device tensors, and out= keeps the steps on the device

KGMT.solution_paths, KGMT.trace and KGMT.trajectories (cudasbmp_amd.kgmt) ask the same of a
planner's own tree.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat

OK, NONE, BROKEN, DEEP = nat.SBMP_PATH_OK, nat.SBMP_PATH_NONE, nat.SBMP_PATH_BROKEN, nat.SBMP_PATH_DEEP


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def paths_dict(call, nodes) -> dict:
    """The two calls of a paths entry point (size, then fill) as KGMT.solution_paths returns them.
    call(lengths, status, rows, samples, costs, capacity, total) makes one."""
    Q = len(nodes)
    lengths = np.zeros(max(1, Q), dtype=np.int32)
    status = np.zeros(max(1, Q), dtype=np.uint8)
    total = ctypes.c_longlong()
    call(_vp(lengths), _vp(status), None, None, None, 0, ctypes.byref(total))
    T = total.value
    rows = np.zeros(max(1, T), dtype=np.int32)
    samples = np.zeros((max(1, T), 7), dtype=np.float32)
    costs = np.zeros(max(1, T), dtype=np.float32)
    if T:
        call(_vp(lengths), _vp(status), _vp(rows), _vp(samples), _vp(costs), T, ctypes.byref(total))
    offsets = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum(lengths[:Q], out=offsets[1:])
    return {"lengths": lengths[:Q], "status": status[:Q], "offsets": offsets, "rows": rows[:T], "samples": samples[:T],
            "costs": costs[:T]}


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr")


def _args(numDisc, agentLength, agent, depthBound):
    a = nat.TreePathsArgs()
    a.depthBound, a.numDisc, a.agentLength = int(depthBound), int(numDisc), float(agentLength)
    a.agent = nat.SBMP_AGENT_POINT if agent == "point" else nat.SBMP_AGENT_CAR
    return a


def _host_tree(state, ctrl, parent):
    host = {"state": np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4),
            "ctrl": np.ascontiguousarray(ctrl, dtype=np.float32).reshape(-1, 4),
            "parent": np.ascontiguousarray(parent, dtype=np.int32).ravel()}
    R = len(host["state"])
    if len(host["ctrl"]) != R or len(host["parent"]) != R:
        raise ValueError("state, ctrl and parent must have the same number of rows")
    return host, R


def tree_paths_batch(state, ctrl, parent, nodes, *, depthBound=0, device=True) -> dict:
    """state (R, 4), ctrl (R, 4), parent (R,): the planner's tree layout; nodes (Q,) int32 rows, -1
    for none.  depthBound: the most rows a path may hold, 0 for R.  Returns lengths, status
    (SBMP_PATH_*), offsets (Q + 1, int64), rows, samples (total, 7) and costs."""
    from .batch import _Dev
    host, R = _host_tree(state, ctrl, parent)
    nodes = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
    a = _args(1, 1.0, "car", depthBound)
    a.rows = R
    devs = {}
    try:
        for name, arr in host.items():
            if device:
                devs[name] = _Dev(arr)
                setattr(a, name, devs[name].ptr)
            else:
                setattr(a, name, arr.ctypes.data)
        n = _vp(nodes) if len(nodes) else None
        if device:
            return paths_dict(lambda *o: nat.call("sbmp_tree_paths_batch", ctypes.byref(a), n, len(nodes), *o, None), nodes)
        return paths_dict(lambda *o: nat.call("sbmp_tree_paths_batch_host", ctypes.byref(a), n, len(nodes), *o), nodes)
    finally:
        for d in devs.values():
            d.close()


def tree_trace_batch(state, ctrl, parent, rows=None, *, count=None, numDisc=10, agentLength=1.0, agent="car",
                     device=True, out=None, stream=None):
    """The numDisc Euler states of the edge that ends on each listed row (rows None: the rows
    [0, count), count None: every row).  Returns (steps (count, numDisc, 4), a transposed view of
    the step-major array, status (count,) uint8 of SBMP_ROW_FREE / ORPHAN / STALE).
    state, ctrl, parent and rows may be device arrays (torch tensors on the GPU, float32 (R, 4) and
    int32: anything cudasbmp_amd.kgmt.device_ptr takes that has a shape) in place of numpy arrays.
    out=(steps, status): device memory for numDisc x count x 4 float32 and count uint8 (torch
    tensors, DeviceBuffers or addresses) that receives the result step-major and keeps it on the
    device; `out` is returned as it is (steps.view(numDisc, count, 4).transpose(0, 1) is the
    (count, numDisc, 4) view of a torch tensor)."""
    from .batch import _Dev
    from .kgmt import device_ptr
    on_device = _is_device(state)
    if on_device and not device:
        raise ValueError("device tensors need device=True")
    a = _args(numDisc, agentLength, agent, 0)
    devs = {}
    try:
        if on_device:
            R = int(state.shape[0])
            a.state, a.ctrl, a.parent = device_ptr(state), device_ptr(ctrl), device_ptr(parent)
        else:
            host, R = _host_tree(state, ctrl, parent)
            for name, arr in host.items():
                if device:
                    devs[name] = _Dev(arr)
                    setattr(a, name, devs[name].ptr)
                else:
                    setattr(a, name, arr.ctypes.data)
        a.rows = R
        if rows is None:
            n = R if count is None else int(count)
            rows_ptr = None
        elif _is_device(rows):
            n = int(np.prod(rows.shape))
            rows_ptr = device_ptr(rows)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            n = len(rows)
            if device and n:
                devs["rows"] = _Dev(rows)
                rows_ptr = devs["rows"].ptr
            else:
                rows_ptr = rows.ctypes.data if n else None
        if out is not None:
            steps_t, status_t = out
            if hasattr(steps_t, "numel") and (steps_t.numel() != numDisc * n * 4 or status_t.numel() != n):
                raise ValueError("out must hold numDisc x count x 4 floats and count bytes")
            nat.call("sbmp_tree_trace_batch", ctypes.byref(a), ctypes.c_void_p(rows_ptr), n,
                     ctypes.c_void_p(device_ptr(steps_t)), ctypes.c_void_p(device_ptr(status_t)),
                     ctypes.c_void_p(stream or 0))
            return out
        steps = np.zeros((numDisc, max(1, n), 4), dtype=np.float32)
        status = np.zeros(max(1, n), dtype=np.uint8)
        if device and n:
            devs["steps"] = _Dev(steps[:, :n])
            devs["status"] = _Dev(status[:n])
            nat.call("sbmp_tree_trace_batch", ctypes.byref(a), ctypes.c_void_p(rows_ptr), n,
                     ctypes.c_void_p(devs["steps"].ptr), ctypes.c_void_p(devs["status"].ptr), ctypes.c_void_p(stream or 0))
            steps, status = devs["steps"].get(), devs["status"].get()
        else:
            nat.call("sbmp_tree_trace_batch_host", ctypes.byref(a), ctypes.c_void_p(rows_ptr), n, _vp(steps), _vp(status))
        return steps[:, :n].transpose(1, 0, 2), status[:n]
    finally:
        for d in devs.values():
            d.close()

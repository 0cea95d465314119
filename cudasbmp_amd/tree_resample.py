"""Solution paths resampled at a fixed period (include/sbmp/tree_resample.h) over
numpy arrays.

    tree_resample_batch   k_path_walk, k_resample_clock and k_path_resample over caller rows on the
                          GPU (sbmp_tree_resample_batch), or, with device=False, the host loop that
                          applies the literal rule (sbmp_tree_resample_batch_host)

KGMT.resample (cudasbmp_amd.kgmt) asks the same of a planner's own tree.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat
from .tree_paths import _args, _host_tree, _vp


def _empty(T):
    return (np.zeros((max(1, T), 4), dtype=np.float32), np.zeros(max(1, T), dtype=np.int32),
            np.zeros(max(1, T), dtype=np.float64))


def resample_dict(call, nodes, fill=None) -> dict:
    """The two calls of a resample entry point (size, then fill) as KGMT.resample returns them.
    call(counts, status, states, edges, times, capacity, total) makes one with host outputs;
    fill(counts, status, T, total) -> (states, edges, times), when given, makes the second."""
    Q = len(nodes)
    counts = np.zeros(max(1, Q), dtype=np.int32)
    status = np.zeros(max(1, Q), dtype=np.uint8)
    total = ctypes.c_longlong()
    call(_vp(counts), _vp(status), None, None, None, 0, ctypes.byref(total))
    T = total.value
    states, edges, times = _empty(T)
    if T:
        if fill is not None:
            states, edges, times = fill(counts, status, T, total)
        else:
            call(_vp(counts), _vp(status), _vp(states), _vp(edges), _vp(times), T, ctypes.byref(total))
    offsets = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum(counts[:Q], out=offsets[1:])
    return {"counts": counts[:Q], "status": status[:Q], "offsets": offsets, "states": states[:T], "edges": edges[:T],
            "times": times[:T]}


def tree_resample_batch(state, ctrl, parent, nodes, period, *, numDisc=10, agentLength=1.0, agent="car", depthBound=0,
                        device=True, stream=None) -> dict:
    """state (R, 4), ctrl (R, 4), parent (R,): the planner's tree layout; nodes (Q,) int32 rows, -1
    for none; period: seconds between two set-points, finite and > 0.  Returns counts (Q,), status
    (Q,) of SBMP_PATH_*, offsets (Q + 1, int64), states (total, 4) of (x, y, theta, v), edges
    (total,) and times (total,) float64; path i is [offsets[i], offsets[i + 1])."""
    from .batch import _Dev
    host, R = _host_tree(state, ctrl, parent)
    nodes = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
    a = _args(numDisc, agentLength, agent, depthBound)
    a.rows = R
    period = ctypes.c_double(float(period))
    devs = {}
    try:
        for name, arr in host.items():
            if device:
                devs[name] = _Dev(arr)
                setattr(a, name, devs[name].ptr)
            else:
                setattr(a, name, arr.ctypes.data)
        n = _vp(nodes) if len(nodes) else None
        if not device:
            return resample_dict(lambda *o: nat.call("sbmp_tree_resample_batch_host", ctypes.byref(a), n, len(nodes),
                                                     period, *o), nodes)

        def on_device(counts, status, states, edges, times, capacity, total):
            nat.call("sbmp_tree_resample_batch", ctypes.byref(a), n, len(nodes), period, counts, status, states, edges,
                     times, capacity, total, ctypes.c_void_p(stream or 0))

        def fill(counts, status, T, total):
            states, edges, times = _empty(T)
            out = [_Dev(states[:T]), _Dev(edges[:T]), _Dev(times[:T])]
            try:
                on_device(_vp(counts), _vp(status), *(ctypes.c_void_p(d.ptr) for d in out), T, ctypes.byref(total))
                return tuple(d.get() for d in out)
            finally:
                for d in out:
                    d.close()

        return resample_dict(on_device, nodes, fill)
    finally:
        for d in devs.values():
            d.close()

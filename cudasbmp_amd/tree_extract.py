"""The usable subtree of a grown tree as a tree of its own: prune and re-root
(include/sbmp/tree_extract.h) over numpy arrays.

    tree_extract_batch   the k_extract_* kernels over caller rows on the GPU (sbmp_tree_extract_batch),
                         or, with device=False, the host loop that applies the literal rule
                         (sbmp_tree_extract_batch_host)
    tree_extract_info    the launcher's seams: rows per tile, tiles per round of the offsets
                         workgroup, and the tiles and rounds of a row count (host-only)

KGMT.extract (cudasbmp_amd.kgmt) asks the same of a planner's own tree.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat
from .tree_paths import _host_tree, _vp

SUMMARY_FIELDS = tuple(k for k, _ in nat.TreeExtract._fields_)


def tree_extract_info(rows: int = 0) -> dict:
    info = nat.TreeExtractLayout()
    nat.call("sbmp_tree_extract_info", int(rows), ctypes.byref(info))
    return {k: getattr(info, k) for k, _ in nat.TreeExtractLayout._fields_}


def _outputs(kept):
    n = max(1, kept)
    return {"state": np.zeros((n, 4), dtype=np.float32), "ctrl": np.zeros((n, 4), dtype=np.float32),
            "parent": np.zeros(n, dtype=np.int32), "origin": np.zeros(n, dtype=np.int32)}


def extract_dict(call, R, fill=None) -> dict:
    """The two calls of an extract entry point (size, then fill) as KGMT.extract returns them.
    call(state, ctrl, parent, origin, newRow, capacity, out) makes one with host outputs;
    fill(kept, out) -> (state, ctrl, parent, origin, newRow), when given, makes the second."""
    s = nat.TreeExtract()
    call(None, None, None, None, None, 0, ctypes.byref(s))
    kept = s.kept
    R = R if R is not None else s.rows
    newRow = np.full(max(1, R), -1, dtype=np.int32)
    o = _outputs(kept)
    if fill is not None:
        o["state"], o["ctrl"], o["parent"], o["origin"], newRow = fill(kept, s)
    else:
        call(_vp(o["state"]), _vp(o["ctrl"]), _vp(o["parent"]), _vp(o["origin"]), _vp(newRow), kept, ctypes.byref(s))
    out = {k: v[:kept] for k, v in o.items()}
    out["newRow"] = newRow[:R]
    out["summary"] = {k: getattr(s, k) for k in SUMMARY_FIELDS}
    return out


def tree_extract_batch(state, ctrl, parent, *, root=0, keep=None, depthBound=0, device=True, stream=None) -> dict:
    """state (R, 4), ctrl (R, 4), parent (R,): the planner's tree layout; root: a row of [0, R);
    keep: (R,) bytes, a row is kept iff its byte is non-zero (None: every row).  depthBound: an
    upper bound on the rows of any parent chain, 0 for R.  Returns state (kept, 4), ctrl (kept, 4),
    parent (kept,), origin (kept,) (the old row of every new row), newRow (R,) (-1 for a row that
    is no member) and summary, a dict rows, kept, below, masked, detached, root, rootCost."""
    from .batch import _Dev
    host, R = _host_tree(state, ctrl, parent)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8).ravel()
        if len(keep) != R:
            raise ValueError("keep must have one byte per row")
    a = nat.TreeExtractArgs()
    a.rows, a.depthBound = R, int(depthBound)
    devs = {}
    try:
        for name, arr in host.items():
            if device and R:
                devs[name] = _Dev(arr)
                setattr(a, name, devs[name].ptr)
            else:
                setattr(a, name, arr.ctypes.data if R else None)
        if not device:
            k = _vp(keep) if keep is not None else None
            return extract_dict(lambda *o: nat.call("sbmp_tree_extract_batch_host", ctypes.byref(a), int(root), k, *o), R)
        if keep is not None and R:
            devs["keep"] = _Dev(keep)
        k = ctypes.c_void_p(devs["keep"].ptr) if "keep" in devs else None

        def on_device(st, ct, pa, og, nr, capacity, out):
            nat.call("sbmp_tree_extract_batch", ctypes.byref(a), int(root), k, st, ct, pa, og, nr, capacity, out,
                     ctypes.c_void_p(stream or 0))

        def fill(kept, s):
            o = _outputs(kept)
            names = ("state", "ctrl", "parent", "origin")
            out = [_Dev(o[n][:kept]) if kept else None for n in names] + [_Dev(np.full(R, -1, dtype=np.int32))]
            try:
                on_device(*(ctypes.c_void_p(d.ptr) if d else None for d in out), kept, ctypes.byref(s))
                return tuple(d.get() if d else o[n] for d, n in zip(out, names + ("newRow",)))
            finally:
                for d in out:
                    if d:
                        d.close()

        return extract_dict(on_device, R, fill)
    finally:
        for d in devs.values():
            d.close()

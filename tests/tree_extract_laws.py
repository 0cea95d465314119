"""The commutation laws of the tree extraction, each stated over origin / newRow and run through
the library's other grown-tree entries: with device=False through their host twins
(tests/test_tree_extract.py), with device=True through the kernels (tests/test_gpu_tree_extract.py).

`tree` holds state, ctrl, parent and params (a tests/tree_recheck_cases.py Case); `ext` is an
extraction of it (a dict as tree_extract_batch returns) with `root` and the keep mask `keep`.
"""
from __future__ import annotations

import numpy as np

from tree_extract_model import members_of, u32

GOALS = np.array([[2.0, 18.0, 0.5], [5.0, 5.0, 0.5], [19.9, 0.1, 0.001], [12.0, 3.0, 2.0], [-3.0, -3.0, 0.5],
                  [9.0, 7.0, 0.5], [10.0, 10.0, np.inf], [10.0, 10.0, 0.0], [15.0, 15.0, 3.0], [5.0, 15.0, 1.5]], np.float32)


def _params(tree):
    p = tree.params
    return dict(numDisc=p["numDisc"], agentLength=p["agentLength"], agent=p["agent"])


def _map(origin, rows):
    """Extracted row numbers as the original's, -1 kept."""
    rows = np.asarray(rows)
    return np.where(rows >= 0, origin[np.maximum(rows, 0)], -1)


def query_law(tree, ext, root, keep, device, goals=GOALS):
    """The query over the extraction equals the masked query over the original, with the member
    byte as mask: count, bestCost and nearestDistance as bits, the rows through origin."""
    from cudasbmp_amd import tree_query_batch
    member, _ = members_of(tree.parent, root, keep)
    assert member.any()
    got = tree_query_batch(ext["state"], ext["ctrl"], goals, device=device)
    want = tree_query_batch(tree.state, tree.ctrl, goals, alive=member.astype(np.uint8), device=device)
    assert np.array_equal(got["count"], want["count"])
    for k in ("bestCost", "nearestDistance"):
        assert np.array_equal(u32(got[k]), u32(want[k])), k
    for k in ("firstRow", "bestRow", "nearestRow"):
        assert np.array_equal(_map(ext["origin"], got[k]), want[k]), k
    return want


def paths_law(tree, ext, root, nodes, device):
    """The path of newRow[node] over the extraction is the original path of node from root onward,
    mapped.  nodes: members whose original path from row 0 is whole."""
    from cudasbmp_amd import tree_paths_batch
    nodes = np.asarray(nodes, np.int32)
    assert np.all(ext["newRow"][nodes] >= 0)
    got = tree_paths_batch(ext["state"], ext["ctrl"], ext["parent"], ext["newRow"][nodes], device=device)
    want = tree_paths_batch(tree.state, tree.ctrl, tree.parent, nodes, device=device)
    assert np.all(got["status"] == 0) and np.all(want["status"] == 0)
    for i in range(len(nodes)):
        g = slice(got["offsets"][i], got["offsets"][i + 1])
        w_rows = want["rows"][want["offsets"][i]:want["offsets"][i + 1]]
        at = int(np.flatnonzero(w_rows == root)[0])
        w = slice(want["offsets"][i] + at, want["offsets"][i + 1])
        assert np.array_equal(ext["origin"][got["rows"][g]], want["rows"][w]), nodes[i]
        assert np.array_equal(u32(got["samples"][g]), u32(want["samples"][w]))
        assert np.array_equal(u32(got["costs"][g]), u32(want["costs"][w]))


def trace_law(tree, ext, device):
    """The trace of every extracted row k > 0 equals the original trace of origin[k]."""
    from cudasbmp_amd import tree_trace_batch
    kept = len(ext["origin"])
    if kept < 2:
        return
    ks = np.arange(1, kept, dtype=np.int32)
    gs, gst = tree_trace_batch(ext["state"], ext["ctrl"], ext["parent"], ks, device=device, **_params(tree))
    ws, wst = tree_trace_batch(tree.state, tree.ctrl, tree.parent, ext["origin"][1:], device=device, **_params(tree))
    assert np.array_equal(u32(np.ascontiguousarray(gs)), u32(np.ascontiguousarray(ws))) and np.array_equal(gst, wst)


def resample_law(tree, ext, nodes, period, device):
    """For root = 0 the resampled paths are byte-identical apart from the edges' renumbering."""
    from cudasbmp_amd import tree_resample_batch
    nodes = np.asarray(nodes, np.int32)
    got = tree_resample_batch(ext["state"], ext["ctrl"], ext["parent"], ext["newRow"][nodes], period, device=device,
                              **_params(tree))
    want = tree_resample_batch(tree.state, tree.ctrl, tree.parent, nodes, period, device=device, **_params(tree))
    for k in ("counts", "status", "offsets", "states", "times"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(ext["origin"][got["edges"]], want["edges"]) and len(got["times"]) > len(nodes)


def recheck_law(tree, device):
    """The extraction taken with the alive mask of a re-check against a list is alive, row for row,
    against that list.  Returns (the extraction, the re-check's summary)."""
    from cudasbmp_amd import tree_extract_batch, tree_recheck_batch
    kw = dict(tree.params)
    status, summary = tree_recheck_batch(tree.state, tree.ctrl, tree.parent, tree.boxes, device=device, **kw)
    alive = (status == 0).astype(np.uint8)
    ext = tree_extract_batch(tree.state, tree.ctrl, tree.parent, keep=alive, device=device)
    assert ext["summary"]["kept"] == summary["alive"] == int(alive.sum()) and ext["summary"]["detached"] == 0
    assert np.array_equal(ext["origin"], np.flatnonzero(alive))
    st2, s2 = tree_recheck_batch(ext["state"], ext["ctrl"], ext["parent"], tree.boxes, device=device, **kw)
    assert np.all(st2 == 0) and s2["alive"] == s2["rows"] == summary["alive"] and s2["firstDead"] == -1
    return ext, summary

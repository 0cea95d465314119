"""A model of the tree extraction (prune and re-root) that shares no code with the library
(include/sbmp/tree_extract.h states the rule the library follows):

  membership   one ascending Python loop: the root is a member iff it is kept; a row above it iff
               it is kept, its parent is a lower row that is not negative, and that parent is a member
  numbering    numpy.cumsum over the member flags
  gather       fancy indexing with the members' rows
  comparisons  on uint32 views, so a NaN, a -0 and a cost all count as their bits

Plain numpy; no GPU, no library.
"""
from __future__ import annotations

import numpy as np

SUMMARY = ("rows", "kept", "below", "masked", "detached", "root")
ARRAYS = ("state", "ctrl", "parent", "origin", "newRow")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def members_of(parent, root, keep=None):
    """(member, kept) flags per row."""
    p = np.asarray(parent).tolist()
    R = len(p)
    kept = [True] * R if keep is None else (np.asarray(keep).astype(np.uint8) != 0).tolist()
    member = [False] * R
    member[root] = kept[root]
    for r in range(root + 1, R):
        q = p[r]
        member[r] = kept[r] and 0 <= q < r and member[q]
    return np.array(member, bool), np.array(kept, bool)


def extract_model(state, ctrl, parent, root=0, keep=None) -> dict:
    state = np.ascontiguousarray(state, np.float32).reshape(-1, 4)
    ctrl = np.ascontiguousarray(ctrl, np.float32).reshape(-1, 4)
    parent = np.ascontiguousarray(parent, np.int32).ravel()
    R = len(parent)
    assert 0 <= root < R
    member, kept = members_of(parent, root, keep)
    newRow = np.where(member, np.cumsum(member) - 1, -1).astype(np.int32)
    origin = np.flatnonzero(member).astype(np.int32)
    old = parent[origin].astype(np.int64)
    if len(origin):
        assert origin[0] == root
        old[0] = root                      # the root's parent word is never read
    newParent = newRow[old].astype(np.int32)
    if len(origin):
        newParent[0] = -1
    rows = np.arange(R)
    below = rows < root
    masked = ~below & ~kept
    detached = ~below & kept & ~member
    summary = {"rows": R, "kept": int(member.sum()), "below": int(below.sum()), "masked": int(masked.sum()),
               "detached": int(detached.sum()), "root": int(root), "rootCost": ctrl[root, 3]}
    return {"state": state[origin], "ctrl": ctrl[origin], "parent": newParent, "origin": origin, "newRow": newRow,
            "summary": summary, "member": member}


def assert_same_extract(got, want, label=""):
    gs, ws = got["summary"], want["summary"]
    assert {k: gs[k] for k in SUMMARY} == {k: ws[k] for k in SUMMARY}, f"{label}: summary {gs} vs {ws}"
    assert u32(np.float32(gs["rootCost"])) == u32(np.float32(ws["rootCost"])), f"{label}: rootCost"
    assert gs["rows"] == gs["kept"] + gs["below"] + gs["masked"] + gs["detached"], f"{label}: {gs}"
    for k in ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, f"{label}: {k} {g.shape} vs {w.shape}"
        if k in ("state", "ctrl"):
            g, w = u32(g), u32(w)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if len(g) else []
        assert len(bad) == 0, f"{label}: {k} differs in {len(bad)} rows, first {bad[:8].tolist()}"

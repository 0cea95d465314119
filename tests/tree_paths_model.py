"""Paths and traces of a grown tree as a model that shares no code with the library
(include/sbmp/tree_paths.h states the rule).

Paths are an explicit parent walk in Python.  The trace is float32 numpy: the transcendentals
are oracle.pyoracle.sincosf / tanf (D9), products and quotients are numpy's own float32
operations (correctly rounded), and fmaf(a, b, c) is float32(float64(a) * float64(b) +
float64(c)): the product is exact in float64, the sum rounds once to float64 and once more to
float32.  The two roundings differ from the single rounding of a fused operation only where
the float64 sum lands within one float64 ulp of a float32 midpoint (or in float32's subnormal
range); those elements are settled with fractions.Fraction, so the model is exact.

    OK 0      the chain node, parent[node], ... reaches row 0 within depthBound rows
    NONE 1    node == -1
    BROKEN 2  a row r > 0 of the chain has no parent in [0, r)
    DEEP 3    more than depthBound rows before either end is met
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

OK, NONE, BROKEN, DEEP = 0, 1, 2, 3
FREE, ORPHAN, STALE = 0, 1, 3


# ---------------------------------------------------------------- paths
def path_of(parent, node, depth_bound):
    """(status, rows root first) of one request."""
    if node == -1:
        return NONE, []
    chain = []
    j = int(node)
    while True:
        if len(chain) + 1 > depth_bound:
            return DEEP, []
        chain.append(j)
        if j == 0:
            return OK, chain[::-1]
        p = int(parent[j])
        if not 0 <= p < j:
            return BROKEN, []
        j = p


def paths_model(state, ctrl, parent, nodes, depth_bound=0) -> dict:
    """What KGMT.solution_paths / tree_paths_batch return, from the walk above."""
    parent = np.asarray(parent)
    bound = depth_bound if depth_bound > 0 else len(parent)
    par = parent.tolist()
    lengths, status, rows = [], [], []
    for n in np.asarray(nodes).tolist():
        st, chain = path_of(par, n, bound)
        status.append(st)
        lengths.append(len(chain))
        rows += chain
    rows = np.array(rows, dtype=np.int32)
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    state = np.asarray(state, np.float32).reshape(-1, 4)
    ctrl = np.asarray(ctrl, np.float32).reshape(-1, 4)
    return {"lengths": np.array(lengths, dtype=np.int32), "status": np.array(status, dtype=np.uint8), "offsets": offsets,
            "rows": rows, "samples": np.concatenate([state[rows], ctrl[rows, :3]], axis=1).astype(np.float32),
            "costs": ctrl[rows, 3].copy()}


def assert_same_paths(got, want, label=""):
    for k in ("lengths", "status", "offsets", "rows"):
        assert np.array_equal(got[k], want[k]), f"{label}: {k} differ"
    for k in ("samples", "costs"):
        g, w = np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(want[k], np.float32)
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{label}: {k} differ"


# ---------------------------------------------------------------- fmaf
def _round_f32(F: Fraction) -> np.float32:
    """F rounded once to the nearest float32, ties to even."""
    with np.errstate(all="ignore"):
        r = np.float32(float(F))                       # within one float32 of the answer
        cands = {float(np.nextafter(r, np.float32(-np.inf))), float(r), float(np.nextafter(r, np.float32(np.inf)))}
    best = None
    for c in sorted(c for c in cands if np.isfinite(c)):
        d = abs(Fraction(c) - F)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return np.float32(best[1])


def fmaf(a, b, c) -> np.ndarray:
    """The fused multiply-add of float32 arrays, exactly."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = s.astype(np.float32)
    low = s.view(np.uint64) & np.uint64((1 << 29) - 1)
    near_mid = (low >= np.uint64((1 << 28) - 1)) & (low <= np.uint64((1 << 28) + 1))
    tiny = (np.abs(s) < 2.0 ** -125) & (s != 0.0)
    doubt = np.isfinite(s) & (near_mid | tiny)
    out = out.copy()
    for i in zip(*np.nonzero(doubt)):
        out[i] = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


# ---------------------------------------------------------------- trace
def euler_steps(parents4, controls3, numDisc, L, agent):
    """(n, numDisc, 4) float32: the state after each Euler step, in the propagator's sequence
    (statePropagator.cu:22-66 without its tests): dt = duration / numDisc, tan(steering) once; per
    step x and y from the old theta and v, then theta (from the old v), then v."""
    from oracle.pyoracle import sincosf, tanf
    p = np.ascontiguousarray(parents4, np.float32).reshape(-1, 4)
    c = np.ascontiguousarray(controls3, np.float32).reshape(-1, 3)
    n = len(p)
    out = np.zeros((n, numDisc, 4), np.float32)
    with np.errstate(all="ignore"):
        dt = c[:, 2] / np.float32(numDisc)
        x, y, th, v = (p[:, i].copy() for i in range(4))
        if agent == "point":
            for j in range(numDisc):
                x = fmaf(c[:, 0], dt, x)
                y = fmaf(c[:, 1], dt, y)
                out[:, j, 0], out[:, j, 1] = x, y
            return out
        a = c[:, 0]
        tan = tanf(c[:, 1])
        LL = np.float32(L)
        for j in range(numDisc):
            sin, cos = sincosf(th)
            x = fmaf(v * cos, dt, x)
            y = fmaf(v * sin, dt, y)
            th = fmaf((v / LL) * tan, dt, th)
            v = fmaf(a, dt, v)
            out[:, j] = np.stack([x, y, th, v], axis=1)
    return out


def trace_model(state, ctrl, parent, rows=None, *, numDisc=10, agentLength=1.0, agent="car", **_):
    """(steps (count, numDisc, 4) float32, status (count,) uint8) of the listed rows (None: all)."""
    state = np.ascontiguousarray(state, np.float32).reshape(-1, 4)
    ctrl = np.ascontiguousarray(ctrl, np.float32).reshape(-1, 4)
    parent = np.ascontiguousarray(parent, np.int32).ravel()
    rows = np.arange(len(state), dtype=np.int64) if rows is None else np.asarray(rows, np.int64).ravel()
    par = parent[rows].astype(np.int64)
    usable = (par >= 0) & (par < rows)
    steps = euler_steps(state[np.where(usable, par, 0)], ctrl[rows, :3], numDisc, agentLength, agent)
    same = (steps[:, -1].view(np.uint32) == state[rows].view(np.uint32)).all(axis=1)
    status = np.where(same, FREE, STALE).astype(np.uint8)
    hold = ~usable | (rows == 0)
    steps[hold] = state[rows[hold], None, :]
    status[~usable] = ORPHAN
    status[rows == 0] = FREE
    return steps, status


def assert_same_trace(got, want, label=""):
    gs, gb = got
    ws, wb = want
    gs, ws = np.ascontiguousarray(gs, np.float32), np.ascontiguousarray(ws, np.float32)
    assert gs.shape == ws.shape, f"{label}: {gs.shape} vs {ws.shape}"
    bad = np.flatnonzero((gs.view(np.uint32) != ws.view(np.uint32)).any(axis=(1, 2)))
    assert len(bad) == 0, f"{label}: {len(bad)} entries differ in their steps, first {bad[:8].tolist()}"
    bad = np.flatnonzero(np.asarray(gb, np.uint8) != np.asarray(wb, np.uint8))
    assert len(bad) == 0, f"{label}: {len(bad)} status bytes differ, first {bad[:8].tolist()}"

"""Solution paths resampled at a fixed period as a model that shares no code with the library
(include/sbmp/tree_resample.h states the rule).

The chain of a request is tree_paths_model.path_of.  The clock is a Python float loop, root first
(Python floats are IEEE doubles).  The edge of a grid time is found with bisect over the clock,
the step j by exact comparison of j * dt (exact in float64) with tau, alpha = float32(tau - j * dt)
computed in float64.  The Euler part is float32 numpy: tree_paths_model.fmaf (exact) and
oracle.pyoracle.sincosf / tanf, in the propagator's sequence, j steps of dt and one of alpha.

`rule` gives the model one of two deliberately wrong readings, for the tests that show the float64
audit notices them:
    "alpha-from-edge-start"   alpha = float32(tau) instead of float32(tau - j * dt)
    "dt-for-alpha"            the last step takes dt instead of alpha
"""
from __future__ import annotations

import bisect
import math

import numpy as np

from tree_paths_model import OK, fmaf, path_of

WRONG_RULES = ("alpha-from-edge-start", "dt-for-alpha")
MAX_RATIO = 2.0 ** 31 - 2


class TooManySamples(ValueError):
    pass


def edge_time(d) -> float:
    d = float(d)
    return d if (d > 0.0 and math.isfinite(d)) else 0.0


def clock_of(ctrl, chain):
    """[T_0, ..., T_{L-1}] of a chain (rows root first), accumulated root first."""
    T = [0.0]
    for r in chain[1:]:
        T.append(T[-1] + edge_time(ctrl[r, 2]))
    return T


def count_of(T, period) -> int:
    q = T / period
    if not q < MAX_RATIO:
        raise TooManySamples(f"T / period = {q}")
    return math.floor(q) + 2


def resample_model(state, ctrl, parent, nodes, period, *, numDisc=10, agentLength=1.0, agent="car", depth_bound=0,
                   rule="", details=False, pick=None, **_):
    """What KGMT.resample / tree_resample_batch return.  details=True adds, per sample: `from` (the
    row the edge starts at, -1 for an end sample), `j`, `alpha` and `dt`.  pick(n): the ascending
    sample numbers of a path of n samples to compute (for a path too long to model whole); counts
    and offsets still speak of whole paths, the sample arrays hold the picked samples only."""
    from oracle.pyoracle import sincosf, tanf
    assert rule in ("",) + WRONG_RULES
    state = np.ascontiguousarray(state, np.float32).reshape(-1, 4)
    ctrl = np.ascontiguousarray(ctrl, np.float32).reshape(-1, 4)
    par = np.asarray(parent).tolist()
    period = float(period)
    assert period > 0.0 and math.isfinite(period)
    bound = depth_bound if depth_bound > 0 else len(par)
    D = int(numDisc)
    counts, status = [], []
    start, edges, times, taus = [], [], [], []      # per sample; start -1: an end sample
    for node in np.asarray(nodes).tolist():
        st, chain = path_of(par, node, bound)
        status.append(st)
        if st != OK:
            counts.append(0)
            continue
        T = clock_of(ctrl, chain)
        n = count_of(T[-1], period)
        counts.append(n)
        for m in (range(n) if pick is None else pick(n)):
            if m == n - 1:
                break
            t = m * period
            k = bisect.bisect_right(T, t)            # the smallest k with t < T[k]; T[0] = 0 <= t
            if k >= len(chain):
                start.append(-1), edges.append(node), times.append(T[-1]), taus.append(0.0)
            else:
                start.append(chain[k - 1]), edges.append(chain[k]), times.append(t), taus.append(t - T[k - 1])
        if pick is None or n - 1 in pick(n):
            start.append(-1), edges.append(node), times.append(T[-1]), taus.append(0.0)
    start = np.array(start, np.int64)
    edges = np.array(edges, np.int32)
    times = np.array(times, np.float64)
    tau = np.array(taus, np.float64)
    grid = start >= 0
    e = edges.astype(np.int64)
    out = state[e].copy() if len(e) else np.zeros((0, 4), np.float32)
    j_all = np.zeros(len(e), np.int64)
    alpha_all = np.zeros(len(e), np.float32)
    dt_all = np.zeros(len(e), np.float32)
    if grid.any():
        with np.errstate(all="ignore"):
            c = ctrl[e[grid]]
            dt = c[:, 2] / np.float32(D)                                   # float32 / float32
            dt64 = dt.astype(np.float64)
            tg = tau[grid]
            j = np.zeros(len(tg), np.int64)
            for q in range(1, D):                                          # q * dt is exact in float64
                j += (q * dt64 <= tg) & (j == q - 1)
            alpha = (tg - j * dt64).astype(np.float32)
            if rule == "alpha-from-edge-start":
                alpha = tg.astype(np.float32)
            elif rule == "dt-for-alpha":
                alpha = dt.copy()
            p = state[start[grid]]
            x, y, th, v = (p[:, i].copy() for i in range(4))
            if agent == "car":
                tan = tanf(c[:, 1])
                LL = np.float32(agentLength)
            for i in range(int(j.max()) + 1):
                act = i <= j
                h = np.where(i < j, dt, alpha).astype(np.float32)
                if agent == "point":
                    xn, yn = fmaf(c[:, 0], h, x), fmaf(c[:, 1], h, y)
                    x, y = np.where(act, xn, x), np.where(act, yn, y)
                    continue
                sin, cos = sincosf(th)
                xn = fmaf(v * cos, h, x)
                yn = fmaf(v * sin, h, y)
                thn = fmaf((v / LL) * tan, h, th)
                vn = fmaf(c[:, 0], h, v)
                x, y, th, v = (np.where(act, a, b) for a, b in ((xn, x), (yn, y), (thn, th), (vn, v)))
            if agent == "point":
                th, v = np.zeros_like(x), np.zeros_like(x)
            out[grid] = np.stack([x, y, th, v], axis=1).astype(np.float32)
            j_all[grid], alpha_all[grid], dt_all[grid] = j, alpha, dt
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    res = {"counts": np.array(counts, dtype=np.int32), "status": np.array(status, dtype=np.uint8), "offsets": offsets,
           "states": out, "edges": edges, "times": times}
    if details:
        res.update({"from": start, "j": j_all, "alpha": alpha_all, "dt": dt_all})
    return res


def assert_same_resample(got, want, label=""):
    for k in ("counts", "status", "offsets", "edges"):
        assert np.array_equal(got[k], want[k]), f"{label}: {k} differ"
    g, w = np.ascontiguousarray(got["times"], np.float64), np.ascontiguousarray(want["times"], np.float64)
    assert g.shape == w.shape, f"{label}: times {g.shape} vs {w.shape}"
    bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
    assert len(bad) == 0, f"{label}: {len(bad)} times differ, first {bad[:8].tolist()}"
    g, w = np.ascontiguousarray(got["states"], np.float32), np.ascontiguousarray(want["states"], np.float32)
    assert g.shape == w.shape, f"{label}: states {g.shape} vs {w.shape}"
    bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (f"{label}: {len(bad)} of {len(g)} states differ, first {bad[:8].tolist()}: "
                           f"{g[bad[:1]].tolist()} vs {w[bad[:1]].tolist()}")

"""An independent model of the adoption rule (include/sbmp/tree_adopt.h).

It shares no code with the library: the cells are stated in numpy float32 with the divisions
and truncations of tests/region_scenarios.py's independent model (here for any N), the counters
are numpy.bincount, the bits numpy.unique, R1Cov a population count over each R1 cell's bits,
the goal test float32 arithmetic one operation at a time.

Plain numpy; no GPU and no library.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
F64 = np.float64
R1_TABLES = ("R1", "R1Avail", "R1Valid", "R1Invalid", "R1Cov")
SUMMARY = ("rows", "nonFinite", "frontierNonFinite", "outOfGrid", "goalRow", "treeSize", "gLo")


def sizes(width, N, n):
    W = F32(width)
    return F32(W / F32(N)), F32(W / F32(n * N))        # KGMT.cu:13-14


def to_cell(q, count):
    """static_cast<int>(q) with the range test that follows it; -1 for NaN and out of range (D3)."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(q)
        ok = np.isfinite(q) & (t >= 0) & (t < count)
    return np.where(ok, t, -1).astype(np.int64)


def local(v, c, R1Size):
    """RN(v - c R1Size), the reference's contracted multiply-subtract (D10): exact in float64,
    one rounding to float32."""
    return (np.asarray(v, dtype=F64) - np.asarray(c, dtype=F64) * F64(R1Size)).astype(F32)


def cells(x, y, width, N, n):
    """(r1, r2) per row: getR1 and getR2 (KGMT.cu:602-629)."""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    R1Size, R2Size = sizes(width, N, n)
    with np.errstate(all="ignore"):
        cx, cy = to_cell((x / R1Size).astype(F32), N), to_cell((y / R1Size).astype(F32), N)
        in1 = (cx >= 0) & (cy >= 0)
        r1 = np.where(in1, cy * N + cx, -1)
        lx, ly = local(x, np.where(in1, cx, 0), R1Size), local(y, np.where(in1, cy, 0), R1Size)
        px, py = to_cell((lx / R2Size).astype(F32), n), to_cell((ly / R2Size).astype(F32), n)
    in2 = in1 & (px >= 0) & (py >= 0)
    return r1, np.where(in2, r1 * (n * n) + py * n + px, -1)


def in_goal(x, y, goal):
    """inGoalRegion (KGMT.cu:635-638, D18) in float32: sqrt(dx dx + dy dy) < r."""
    if goal is None:
        return np.zeros(len(x), dtype=bool)
    gx, gy, r = (F32(v) for v in goal)
    with np.errstate(all="ignore"):
        dx, dy = (np.asarray(x, dtype=F32) - gx).astype(F32), (np.asarray(y, dtype=F32) - gy).astype(F32)
        d2 = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
        return np.sqrt(d2).astype(F32) < r


def tables(state, width, N, n, goal=None, frontier_from=0) -> dict:
    """The five R1 tables, the R2 bit words and the summary an adoption of `state` leaves."""
    st = np.asarray(state, dtype=F32).reshape(-1, 4)
    R = len(st)
    nR1, nn = N * N, n * n
    nR2 = nR1 * nn
    r1, r2 = cells(st[:, 0], st[:, 1], width, N, n)
    count = np.bincount(r1[r1 >= 0], minlength=nR1).astype(np.int32)
    cellbits = np.zeros(nR2, dtype=np.uint8)
    cellbits[np.unique(r2[r2 >= 0])] = 1
    words = np.zeros((nR2 + 31) // 32 * 32, dtype=np.uint8)
    words[:nR2] = cellbits
    R2bits = (words.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    non_finite = ~np.isfinite(st).all(axis=1)
    inside = np.flatnonzero(in_goal(st[:, 0], st[:, 1], goal))
    out = {"R1": count, "R1Avail": (count > 0).astype(np.int32), "R1Valid": count.copy(),
           "R1Invalid": np.zeros(nR1, dtype=np.int32),
           "R1Cov": cellbits.reshape(nR1, nn).sum(axis=1).astype(np.int32), "R2bits": R2bits}
    out["summary"] = {"rows": R, "nonFinite": int(non_finite.sum()),
                      "frontierNonFinite": int(non_finite[frontier_from:].sum()),
                      "outOfGrid": int(((r1 < 0) | (r2 < 0)).sum()),
                      "goalRow": int(inside[0]) if len(inside) else -1, "treeSize": R, "gLo": int(frontier_from)}
    return out


def seed_root_tables(x, y, width, N, n) -> dict:
    """What the reference leaves after seeding its root (KGMT.cu:85-97), written out from those
    lines: R1[r1] = 1, R1Avail[r1] = 1, R1Valid[r1] = 1 if r1 >= 0 (D3); R2Avail[r2] = 1 and the
    coverage of r2's R1 cell one higher if r2 >= 0; everything else as constructed (zero)."""
    nR1, nn = N * N, n * n
    r1, r2 = cells(np.array([x]), np.array([y]), width, N, n)
    r1, r2 = int(r1[0]), int(r2[0])
    t = {k: np.zeros(nR1, dtype=np.int32) for k in R1_TABLES}
    t["R2bits"] = np.zeros((nR1 * nn + 31) // 32, dtype=np.uint32)
    if r1 >= 0:
        t["R1"][r1] = 1
        t["R1Avail"][r1] = 1
        t["R1Valid"][r1] = 1
    if r2 >= 0:
        t["R2bits"][r2 >> 5] |= np.uint32(1 << (r2 & 31))
        t["R1Cov"][r2 // nn] += 1
    return t


def same_tables(got: dict, want: dict, label="") -> None:
    for k in R1_TABLES + ("R2bits",):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{label}: {k}"
    if "summary" in want and "summary" in got:
        assert got["summary"] == want["summary"], f"{label}: summary {got['summary']} != {want['summary']}"

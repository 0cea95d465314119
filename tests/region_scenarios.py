"""Family J, "region edges": which R1 / R2 cell a child falls in, what the region counters
become, what R1Score becomes and whether the child is accepted -- the step between the
collision verdict (family H) and the goal verdict (family I) -- at the edges of each decision.

The model (`model_cells`, `counters`, `score`, `accept`, `check_iteration`) is float32 numpy written
from the reference's lines (KGMT.cu:386-411 propagateG after propagateAndCheck, 487-538
updateR1, 602-629 getR1 / getR2).  It shares no code with include/, csrc/, oracle/ or
tests/f64_model.py, has no tolerance and excuses no child.  Its inputs are what a stepped
planner (the CPU oracle or the HIP planner alike) shows before and after one iteration: the
child array, S from the iteration log, the RNG states and the region tables.

  validity  In a box-free scene a child is valid iff its stored (x, y) lies inside the workspace
            under the reference's wall comparisons (x <= 0, x >= W, y <= 0, y >= H leave): a child
            that leaves keeps the (x, y) it left with.  Under a covering box no child is valid.
  cells     q = fl(x / R1Size) (numpy's division is correctly rounded), truncated toward zero;
            the cell is -1 outside [0, 16) and for NaN (D3).  lx = RN(x - c R1Size) with one
            rounding (nvcc contracts the line, D10), computed exactly in float64 (a 24-bit by
            4-bit product and a difference of neighbours in magnitude) and rounded once;
            p = fl(lx / R2Size), truncated; -1 outside [0, n).  R1Size = fl(W / 16) and
            R2Size = fl(W / (16 n)) on both axes.
  counters  KGMT.cu:392-411 with D3 (index -1 is out of bounds in the reference and skipped here):
            a child with r1 >= 0 raises R1[r1], and R1Valid[r1] (setting R1Avail[r1]) or
            R1Invalid[r1]; a child with r2 >= 0 likewise raises R2Valid[r2] (setting R2Avail[r2])
            or R2Invalid[r2].  So a child with r1 >= 0 and r2 < 0 (an "R2 gap" child) touches
            the three R1 tables and no R2 table, and is never accepted.
  score     updateR1 in the reference's types: float covR, float freeVol with epsilon = 0.01f,
            (fv fv)(fv fv) in float (D17), the denominator in double, one rounding to float;
            the sum in CUB's order (D8: an offset-1, 2, 4, 8, 16 tree per 32 cells, then the 8
            partial sums in order); a float division by the total; 1.0f where the cell is
            unavailable.  Computed from the counters as the previous iteration left them (D2).
  accept    u is the draw after the three controls, from the RNG state read before the step
            (a numpy XORWOW step, held against tests/golden/xorwow_rocrand_kat.json by the CPU
            module); curand_uniform is x 2^-32 + 2^-33 in float;
            accept = valid && r2 >= 0 && (u <= score[r1] || R2Avail_before[r2] == 0).
            The accepted children in slot order are the inserted rows; a valid child has drawn
            four values, an invalid one three.

Planted cases: seeded searches over iteration 1's children and over widths, classified in exact
rational arithmetic; tests/test_region_scenarios_oracle.py asserts every property claimed.

  J-r1      round-up triples on a child x and a cell line c: the width where the real quotient
            x / R1Size lies below c and its float equals c (cell c: `up`), its one-ulp wider
            neighbour where the float is pred(c) (cell c - 1: `below`), and the nearest narrower
            width where the real quotient lies above c (`above`).  In x and in y on an odd line (n = 8;
            each axis has its own lines in every restatement), and in x for the point agent.  A power-of-two line cannot be reached by rounding up
            (see r1_triples); there the first width, 16 x / c exactly, puts the quotient on c itself
            (`on`): in y (n = 3).  The `up` child has lx = RN(x - c R1Size) < 0 and p in (-1, 0):
            it lands in sub-column 0 of cell c (J-neglx; n > 1).
  J-minus1  a child that left through x < 0 (y < 0): width = -16 x puts the quotient on -1.0, the
            child is not counted (`at`); one ulp wider the quotient lies in (-1, 0) and the
            invalid child is counted in column (row) 0 (`in`); one ulp narrower it is not counted.
  J-fma     a width whose c R1Size is inexact, and a child whose fused and unfused lx fall in
            different R2 cells; n = 3 and n = 8 in x, n = 8 in y.
  J-gap     a valid child with r1 >= 0 and p >= n (R2Size was rounded down), hence r2 = -1;
            n = 11 and n = 12 in x, n = 11 in y.
  branches  the host verifies the reciprocal division per divisor (sbmp_division_reciprocal) and
            bins_k takes it only with both R1Size and R2Size verified.  No width near the targets
            is rejected, but every divisor past 2^20 is: J-r1, J-fma and J-gap are searched at a
            `small` site (widths 12 .. 140, the reciprocal) and at a `large` one (widths past 2^24,
            the IEEE division).
  J-conc    width 4000, root mid-cell, 65,536 slots, 2 iterations: every child in one R1 and one
            R2 cell; box-free (all valid, all accepted) and under a covering box (all invalid,
            the run stalls, D7); n = 4 (the key log) and n = 12 (direct atomics).  With one available
            cell the score is s / s = 1, so J-conc-n4-two-cells puts the root one unit under an R1 line:
            two cells share the children and 1 + R1^2 with R1 past 2^16 shows in the score.
  J-accept  sbmp_expand_batch takes R1Score as an input: for a target child in an available cell
            R1Score[r1] = u, up(u), down(u) gives accept, accept, reject.
  J-root    the root's own binning at begin(): the root planted on a round-up width.

Plain numpy plus the CPU oracle and the library's host-only calls, at call time; no GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from scenarios import Scenario, make_oracle

F32 = np.float32
F64 = np.float64
U32 = np.uint32
N1 = 16                                         # NUM_R1 (KGMT.cu:8)
R1_KEYS = ("R1", "R1Avail", "R1Valid", "R1Invalid")
R2_KEYS = ("R2Avail", "R2Valid", "R2Invalid")


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def ulps(v, k):
    """The positive float32 v moved by k ulps."""
    return (np.asarray(v, dtype=F32).view(np.int32) + np.int32(k)).view(F32)


def no_boxes() -> np.ndarray:
    return np.zeros((0, 4), dtype=np.float32)


def covering_box() -> np.ndarray:
    return np.array([[-1e6, -1e6, 1e6, 1e6]], dtype=np.float32)


# ---------------------------------------------------------------- the model: cells
def sizes(width, n):
    W = F32(width)
    return F32(W / F32(N1)), F32(W / F32(n * N1))       # KGMT.cu:13-14


def to_cell(q, count):
    """static_cast<int>(q) with the range test that follows it; -1 for NaN and out of range (D3)."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(q)
        ok = np.isfinite(q) & (t >= 0) & (t < count)
    return np.where(ok, t, -1).astype(np.int64)


def local(v, c, R1Size):
    """RN(v - c R1Size): exact in float64, one rounding to float32."""
    return (np.asarray(v, dtype=F64) - np.asarray(c, dtype=F64) * F64(R1Size)).astype(F32)


def valid_children(x, y, width, height, covering):
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    if covering:
        return np.zeros(len(x), dtype=bool)
    with np.errstate(invalid="ignore"):
        return ~((x <= 0) | (x >= F32(width)) | (y <= 0) | (y >= F32(height)))


# ---------------------------------------------------------------- the model: counters
def counters(before: dict, r1, r2, valid, n) -> dict:
    """The region tables after the children (r1, r2, valid) are counted (KGMT.cu:392-411, D3)."""
    out = {k: before[k].astype(np.int64) for k in R1_KEYS + R2_KEYS}
    nR1, nR2 = N1 * N1, N1 * N1 * n * n
    a, b = r1 >= 0, r2 >= 0
    out["R1"] += np.bincount(r1[a], minlength=nR1)
    out["R1Valid"] += np.bincount(r1[a & valid], minlength=nR1)
    out["R1Invalid"] += np.bincount(r1[a & ~valid], minlength=nR1)
    out["R1Avail"][np.unique(r1[a & valid])] = 1
    out["R2Valid"] += np.bincount(r2[b & valid], minlength=nR2)
    out["R2Invalid"] += np.bincount(r2[b & ~valid], minlength=nR2)
    out["R2Avail"][np.unique(r2[b & valid])] = 1
    return out


# ---------------------------------------------------------------- the model: score
def cub_sum(s):
    """BlockReduce<float, 256>::Sum in the warp-reductions order (D8)."""
    t = np.array(s, dtype=F32).reshape(8, 32)
    for off in (1, 2, 4, 8, 16):
        t[:, ::2 * off] = t[:, ::2 * off] + t[:, off::2 * off]
    total = t[0, 0]
    for w in range(1, 8):
        total = F32(total + t[w, 0])
    return total


def score(tables: dict, n, total=cub_sum, wide=F64):
    """R1Score as updateR1 (KGMT.cu:487-538) leaves it, from the tables of the previous iteration."""
    avail = tables["R1Avail"] != 0
    covR = F32(0) * np.zeros(N1 * N1, dtype=F32)
    for col in tables["R2Avail"].reshape(N1 * N1, n * n).T:     # covR += R2Avail[i], in index order
        covR = (covR + col.astype(F32)).astype(F32)
    covR = (covR / F32(n * n)).astype(F32)
    eps = F32(0.01)
    nv = (eps + tables["R1Valid"].astype(F32)).astype(F32)
    with np.errstate(all="ignore"):
        fv = (nv / (nv + tables["R1Invalid"].astype(F32)).astype(F32)).astype(F32)
        fv2 = (fv * fv).astype(F32)
        fv4 = (fv2 * fv2).astype(F32)
        r = tables["R1"].astype(wide)             # pow(int, 2) and all that follows it are double
        den = (F32(1) + covR).astype(F32).astype(wide) * (wide(1) + r * r)
        s = np.where(avail, (fv4.astype(wide) / den).astype(F32), F32(0)).astype(F32)
        return np.where(avail, (s / total(s)).astype(F32), F32(1)).astype(F32)


# ---------------------------------------------------------------- the model: XORWOW and accept
def xorwow_step(st):
    """One draw from every state of st (k, 6) uint32 = (v0 .. v4, d): (draws, next states)."""
    st = np.array(st, dtype=U32)
    t = st[:, 0] ^ (st[:, 0] >> U32(2))
    v4 = st[:, 4]
    nv = (v4 ^ (v4 << U32(4))) ^ (t ^ (t << U32(1)))
    d = st[:, 5] + U32(362437)
    return nv + d, np.stack([st[:, 1], st[:, 2], st[:, 3], st[:, 4], nv, d], axis=1)


def uniform(x):
    """curand_uniform of a draw: x 2^-32 + 2^-33 in float (the product is exact)."""
    return ((x.astype(F32) * F32(2.0 ** -32)).astype(F32) + F32(2.0 ** -33)).astype(F32)


CONTROL_DRAWS = 3       # both agents draw two controls and a duration before the accept draw


def accept_draw(rng_before, draws_before=CONTROL_DRAWS):
    """(u, the states after the controls, the states after u)."""
    st = np.array(rng_before, dtype=U32)
    for _ in range(draws_before):
        _, st = xorwow_step(st)
    x, st4 = xorwow_step(st)
    return uniform(x), st, st4


def accept(valid, r1, r2, u, R1Score, R2Avail_before):
    ok = valid & (r2 >= 0)
    with np.errstate(invalid="ignore"):
        return ok & ((u <= R1Score[np.where(ok, r1, 0)]) | (R2Avail_before[np.where(ok, r2, 0)] == 0))


# ---------------------------------------------------------------- the model over one iteration
@dataclass(frozen=True, eq=False)
class Model:
    """What may be swapped for a power test; the defaults are the reference's."""
    quotient: object = staticmethod(lambda v, size: (np.asarray(v, dtype=F32) / F32(size)).astype(F32))
    to_cell: object = staticmethod(to_cell)
    local: object = staticmethod(local)
    total: object = staticmethod(cub_sum)
    wide: object = F64                          # the type of updateR1's denominator
    accept: object = staticmethod(accept)
    draws_before: int = CONTROL_DRAWS
    count_gap_in_R2: bool = False
    y: object = None                            # another Model for the y lines alone (each axis has its own lines)


@dataclass(frozen=True, eq=False)
class Snapshot:
    """A stepped planner between two iterations."""
    logs: np.ndarray
    unexplored: np.ndarray
    uParent: np.ndarray
    rng: np.ndarray
    regions: dict
    samples: np.ndarray
    parents: np.ndarray


def snapshot(p) -> Snapshot:
    """Of the CPU oracle or of the HIP planner (they name the iteration log differently)."""
    logs = p.iter_logs() if hasattr(p, "iter_logs") else p.iter_log()
    u, up_ = p.unexplored()
    s, par, _ = p.tree()
    return Snapshot(logs, u, up_, p.rng(), p.regions(), s, par)


def step(p) -> bool:
    return p.step() if hasattr(p, "iter_logs") else p.step(1)


@dataclass(frozen=True, eq=False)
class Seen:
    """The model's per-child view of one iteration (for the cases' own assertions)."""
    S: int
    x: np.ndarray
    y: np.ndarray
    valid: np.ndarray
    r1: np.ndarray
    r2: np.ndarray
    u: np.ndarray
    score: np.ndarray
    accept: np.ndarray


def model_cells(m: Model, x, y, width, n):
    """(r1, r2, the R2 sub-cell (px, py)) per child: getR1 and getR2 (KGMT.cu:602-629)."""
    R1Size, R2Size = sizes(width, n)
    with np.errstate(all="ignore"):
        my = m.y or m
        cx, cy = m.to_cell(m.quotient(x, R1Size), N1), my.to_cell(my.quotient(y, R1Size), N1)
        in1 = (cx >= 0) & (cy >= 0)
        r1 = np.where(in1, cy * N1 + cx, -1)
        lx, ly = m.local(x, np.where(in1, cx, 0), R1Size), my.local(y, np.where(in1, cy, 0), R1Size)
        px, py = m.to_cell(m.quotient(lx, R2Size), n), my.to_cell(my.quotient(ly, R2Size), n)
    in2 = in1 & (px >= 0) & (py >= 0)
    return r1, np.where(in2, r1 * (n * n) + py * n + px, -1), (px, py)


def check_iteration(case, before: Snapshot, after: Snapshot, m: Model = Model(), label="") -> Seen:
    """One iteration of a stepped planner against the model: counters, score, inserted rows, RNG."""
    n, M = case.n, len(after.parents)
    assert len(after.logs) == len(before.logs) + 1, f"{label}: one more iteration logged"
    log = after.logs[-1]
    ts, S, A, ts_after = int(log[1]), int(log[5]), int(log[6]), int(log[7])
    x, y = after.unexplored[:S, 0].copy(), after.unexplored[:S, 1].copy()
    valid = valid_children(x, y, case.width, case.height, case.covering)
    r1, r2, (px, py) = model_cells(m, x, y, case.width, n)
    if m.count_gap_in_R2:       # an altered model: the gap child counted in the nearest sub-cell
        gap = (r1 >= 0) & (r2 < 0)
        r2 = np.where(gap, r1 * n * n + np.clip(py, 0, n - 1) * n + np.clip(px, 0, n - 1), r2)
    # D2: the score of this iteration comes from the tables the previous one left
    sc = score(before.regions, n, m.total, m.wide)
    assert np.array_equal(after.regions["R1Score"].view(U32), sc.view(U32)), \
        f"{label}: R1Score differs at cells {np.nonzero(after.regions['R1Score'].view(U32) != sc.view(U32))[0][:8]}"
    want = counters(before.regions, r1, r2, valid, n)
    for k in R1_KEYS + R2_KEYS:
        assert np.array_equal(after.regions[k], want[k]), \
            f"{label}: {k} differs at cells {np.nonzero(after.regions[k] != want[k])[0][:8]}"
    u = accept_draw(before.rng[:S], m.draws_before)[0]
    acc = m.accept(valid, r1, r2, u, sc, before.regions["R2Avail"])
    # the accepted children in slot order are the rows ts .. ts + A (the GNew bits, after the complete clear)
    slots = np.nonzero(acc)[0]
    assert A == len(slots) and ts_after == ts + A and ts + A <= M, f"{label}: A {A}, model {len(slots)}"
    assert np.array_equal(after.samples[ts:ts + A].view(U32), after.unexplored[slots].view(U32)), f"{label}: inserted rows"
    assert np.array_equal(after.parents[ts:ts + A], after.uParent[slots]), f"{label}: inserted rows' parents"
    assert np.array_equal(after.samples[:ts].view(U32), before.samples[:ts].view(U32))
    rng = before.rng.copy()
    _, st3, st4 = accept_draw(before.rng[:S])
    rng[:S] = np.where(valid[:, None], st4, st3)      # a valid child has drawn u as well
    assert np.array_equal(after.rng, rng), f"{label}: RNG states"
    return Seen(S, x, y, valid, r1, r2, u, sc, acc)


def trace(case, p) -> list:
    """Step a begun planner to its end: the snapshots before iteration 1 and after every iteration."""
    snaps = [snapshot(p)]
    for _ in range(case.iterations):
        more = step(p)
        snaps.append(snapshot(p))
        if len(snaps[-1].logs) == len(snaps[-2].logs):
            snaps.pop()
            break
        if not more:
            break
    return snaps


def check_trace(case, snaps, m: Model = Model(), label="") -> list:
    """The model on every iteration of a trace; the Seen of each."""
    return [check_iteration(case, a, b, m, f"{label or case.name} iteration {k + 1}")
            for k, (a, b) in enumerate(zip(snaps, snaps[1:]))]


# ---------------------------------------------------------------- cases
@dataclass(frozen=True)
class Site:
    """Where a search looks: a root, the workspace of the pass whose children it searches, and the
    widths it may move the workspace to (the height stays)."""
    name: str
    root: tuple
    width: float
    height: float
    wmin: float
    wmax: float


# a moving root whose children spread over a few R1 cells of every width in reach
SMALL = Site("small", (8.3, 7.1, 0.7, 3.0), 20.0, 20.0, 12.0, 30.0)
# The host verifies the reciprocal for every divisor in [2^-20, 2^20] the searches ever met (Markstein's
# sequence with y = RN(1/b) is exact but for rare divisors), and rejects every divisor outside that
# range unseen.  So the IEEE branch of bins_k is reached through R1Size > 2^20: widths past 2^24, where
# a child's float spacing is 1 and a fast root still gives some hundred distinct coordinates per axis.
# The coordinates lie just under 2^24, where a float's relative spacing is finest (the R2 gap needs that).
LARGE = Site("large", (16609443.0, 16200005.0, 0.7, 60.0), 2.0 ** 25, 2.0 ** 26, 2.0 ** 24 * 1.0625, 2.0 ** 26)
# heading for the corner: children leave through x < 0 and through y < 0
CORNER = Site("corner", (0.45, 0.4, 3.9, 4.0), 20.0, 20.0, 0.0, 20.0)
# An R2 gap child lies within about 2^-24 R1Size of the next R1 line c + 1 and must not be rounded onto
# it, which takes (c + 1) 2^-25 R1Size: only the lines 1 and 2 leave room.  So the gap searches move the
# same roots into workspaces wide enough to put them in cell 0 or 1.
SMALL_WIDE = Site("small", SMALL.root, SMALL.width, SMALL.height, 40.0, 140.0)
LARGE_WIDE = Site("large", LARGE.root, LARGE.width, LARGE.height, 2.0 ** 26, 2.0 ** 29)
CONC_LINE_ROOT = (1249.0, 1093.75, 0.0, 0.0)    # one unit under the line between R1 columns 4 and 5
CONC_ROOT = (1093.75, 1093.75, 0.0, 0.0)        # width 4000: the middle of R1 cell (4, 4) and of a sub-cell for n = 4 and 12


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    width: float
    n: int
    root: tuple = SMALL.root
    seed: int = 5
    agent: str = "car"
    covering: bool = False
    slots: int = 16384
    iterations: int = 3
    height: float = SMALL.height
    target: int = -1                            # the planted child's slot in iteration 1
    axis: int = 0
    c: int = -1                                 # the cell line
    kind: str = ""
    site: str = "small"

    def __str__(self):
        return self.name


def scenario(case: Case, env=None, local_group: int = 0) -> Scenario:
    kw = dict(width=float(case.width), height=float(case.height), n=case.n, samplesPerIteration=case.slots,
              numIterations=case.iterations, agent=case.agent, maxTreeSize=case.slots * case.iterations + 1)
    return Scenario(name=case.name, family="J", targets="region edges", kw=kw,
                    boxes=covering_box if case.covering else no_boxes, initial=case.root, goal=(-100.0, -100.0),
                    seed=case.seed, env=dict(env or {}), local_group=local_group)


@functools.lru_cache(maxsize=None)
def children1(site: Site, agent, width, seed=5):
    """Iteration 1's children of the site's box-free scene at `width` ((S, 2) float32) and which are valid."""
    c = Case("search", float(width), 1, site.root, seed, agent, iterations=1, height=site.height)
    o = make_oracle(scenario(c), plan=False)
    o.step()
    u, _ = o.unexplored()
    xy = u[:int(o.iter_logs()[0, 5]), :2].copy()
    v = valid_children(xy[:, 0], xy[:, 1], width, site.height, False)
    xy.setflags(write=False)
    return xy, v


def same_child(site, agent, width, slot, value, axis) -> bool:
    """The child of `slot` keeps its float and stays valid at another width."""
    xy, v = children1(site, agent, float(width))
    return bool(v[slot]) and F32(xy[slot, axis]).view(U32) == F32(value).view(U32)


def firsts(v, mask):
    """The slots of mask that hold the first occurrence of their value, ascending."""
    idx = np.nonzero(mask)[0]
    _, first = np.unique(v[idx], return_index=True)
    return idx[np.sort(first)]


def exact_quotient(v, width) -> Fraction:
    return Fraction(float(F32(v))) / Fraction(float(sizes(width, 1)[0]))


def branch(width, n) -> str:
    """The division bins_k takes at this width: `rcp` with both divisors verified by the host, else `ieee`."""
    from cudasbmp_amd.kgmt import division_reciprocal
    R1Size, R2Size = sizes(width, n)
    return "rcp" if division_reciprocal(float(R1Size)) != 0.0 and division_reciprocal(float(R2Size)) != 0.0 else "ieee"


@dataclass(frozen=True)
class Triple:
    slot: int
    axis: int
    c: int
    value: float            # the child's coordinate
    first: str              # `up`: the real quotient below c, its float on c; `on`: the quotient is c exactly
    up: float               # the three widths
    below: float
    above: float


def round_up_widths(v, c):
    """Per element of v (float32), the widths within 3 ulps of fl(16 v / c) at which the real quotient
    lies below c and its float equals c (float64 screens; the caller confirms in rationals)."""
    v = np.asarray(v, dtype=F32)
    W0 = (F32(16) * v / F32(c)).astype(F32)
    out = []
    for k in range(-3, 4):
        W = ulps(W0, k)
        R1Size = (W / F32(16)).astype(F32)
        hit = ((v / R1Size).astype(F32) == F32(c)) & (v.astype(F64) / R1Size.astype(F64) < c)
        out.append((W, hit))
    return out


@functools.lru_cache(maxsize=None)
def r1_triples(site: Site, agent, axis, cs, limit=4) -> tuple:
    """Up to `limit` triples per cell line of `cs` on iteration 1's valid children, by slot.  For an odd
    line the first width rounds the quotient up onto c.  For a power-of-two line that cannot happen (with
    v = m_v 2^a and W = m_W 2^b the quotient is c (m_v / m_W) 2^k, and a ratio of two 24-bit integers
    below 1 lies at least 2^-24 below it, more than the half ulp under a power of two): there the first
    width, 16 v / c exactly, puts the quotient on c itself."""
    xy, valid = children1(site, agent, site.width)
    v = xy[:, axis]
    found = []
    for c in cs:
        if c & (c - 1) == 0:
            W = (F32(16) * v / F32(c)).astype(F32)      # exact: a power-of-two scale
            cand = [(int(s), float(W[s])) for s in firsts(v, valid & (W >= site.wmin) & (W <= site.wmax))]
        else:
            cand = sorted((int(s), float(W[s])) for W, hit in round_up_widths(v, c)
                          for s in firsts(v, hit & valid & (W >= site.wmin) & (W <= site.wmax)))
        got = 0
        for s, W in cand:
            if got == limit:
                break
            q = exact_quotient(v[s], W)
            first = "on" if q == c else "up"
            if not (q <= c and F32(v[s]) / sizes(W, 1)[0] == F32(c)) or (first == "on") != (c & (c - 1) == 0):
                continue
            below = float(up(W))
            above = next((float(ulps(W, -k)) for k in range(1, 8) if exact_quotient(v[s], ulps(W, -k)) > c), None)
            if above is None or to_cell(F32(v[s]) / sizes(below, 1)[0], N1) != c - 1:
                continue
            if all(same_child(site, agent, w, s, v[s], axis) for w in (W, below, above)):
                found.append(Triple(s, axis, c, float(v[s]), first, W, below, above))
                got += 1
    return tuple(found)


@dataclass(frozen=True)
class Planted:
    slot: int
    axis: int
    c: int
    value: float
    width: float
    n: int


def unfused_local(v, c, R1Size):
    """x - fl(c R1Size): the line without nvcc's contraction (two roundings)."""
    return (np.asarray(v, dtype=F32) - (np.asarray(c, dtype=F32) * F32(R1Size)).astype(F32)).astype(F32)


def _near_lines(x, lines, per_line):
    """The widths within 4 ulps of fl(per_line x / line), flat."""
    W0 = (F32(per_line) * F32(x) / lines.astype(F32)).astype(F32)
    return ulps(W0[:, None], np.arange(-4, 5)[None, :]).ravel()


@functools.lru_cache(maxsize=None)
def fma_cases(site: Site, n, axis=0, limit=3, children=1500) -> tuple:
    """Children and widths at which the fused and the unfused lx fall in different R2 cells, both in
    [0, n), on an inexact c R1Size: the widths that put the child near a sub-cell line."""
    xy, valid = children1(site, "car", site.width)
    v = xy[:, axis]
    found = []
    for s in firsts(v, valid)[:children]:
        x = F32(v[s])
        lo, hi = int(16 * n * float(x) / site.wmax) + 1, int(16 * n * float(x) / site.wmin)
        m = np.array([k for k in range(lo, hi + 1) if k % n and n <= k < 16 * n], dtype=np.int64)
        if not len(m):
            continue
        W = _near_lines(x, m, 16 * n)
        W = W[(W >= site.wmin) & (W <= site.wmax)]
        R1Size, R2Size = (W / F32(16)).astype(F32), (W / F32(16 * n)).astype(F32)
        c = to_cell((x / R1Size).astype(F32), N1)
        ok = c >= 1
        cc = np.where(ok, c, 0)
        prod = cc.astype(F64) * R1Size.astype(F64)
        lf, lu = local(x, cc, R1Size), unfused_local(x, cc, R1Size)
        pf, pu = to_cell((lf / R2Size).astype(F32), n), to_cell((lu / R2Size).astype(F32), n)
        for i in np.nonzero(ok & (pf != pu) & (pf >= 0) & (pu >= 0) & (prod != prod.astype(F32)))[0]:
            if same_child(site, "car", float(W[i]), int(s), x, axis):
                found.append(Planted(int(s), axis, int(c[i]), float(x), float(W[i]), n))
                break
        if len(found) >= limit:
            break
    return tuple(found)


@functools.lru_cache(maxsize=None)
def gap_cases(site: Site, n, axis=0, limit=3, children=1500) -> tuple:
    """Valid children with r1 >= 0 and fl(lx / R2Size) >= n: the widths that put the child just below
    the next R1 line, where n R2Size < R1Size leaves a gap."""
    xy, valid = children1(site, "car", site.width)
    v = xy[:, axis]
    found = []
    for s in firsts(v, valid)[:children]:
        x = F32(v[s])
        lo, hi = int(16 * float(x) / site.wmax) + 1, int(16 * float(x) / site.wmin)
        lines = np.arange(max(lo, 1), min(hi, 15) + 1)
        if not len(lines):
            continue
        W = _near_lines(x, lines, 16)
        W = W[(W >= site.wmin) & (W <= site.wmax)]
        R1Size, R2Size = (W / F32(16)).astype(F32), (W / F32(16 * n)).astype(F32)
        c = to_cell((x / R1Size).astype(F32), N1)
        ok = c >= 0
        p = np.trunc((local(x, np.where(ok, c, 0), R1Size) / R2Size).astype(F32))
        for i in np.nonzero(ok & (p >= n))[0]:
            if same_child(site, "car", float(W[i]), int(s), x, axis):
                found.append(Planted(int(s), axis, int(c[i]), float(x), float(W[i]), n))
                break
        if len(found) >= limit:
            break
    return tuple(found)


@functools.lru_cache(maxsize=None)
def minus_one(axis) -> Planted:
    """The first child of the corner root (by slot) that left through the low wall of `axis` alone and
    keeps its float in the three narrow workspaces round width = -16 v."""
    xy, _ = children1(CORNER, "car", CORNER.width)
    v, other = xy[:, axis], xy[:, 1 - axis]
    for s in np.nonzero((v < 0) & (other > 0))[0]:
        W = F32(-16) * F32(v[s])
        if all(F32(children1(CORNER, "car", float(w))[0][s, axis]).view(U32) == F32(v[s]).view(U32)
               for w in (W, up(W), down(W))):
            return Planted(int(s), axis, 0, float(v[s]), float(W), 1)
    raise AssertionError("no child leaves through the low wall alone")


ODD = (3, 5, 7, 9, 11, 13)
R1_SEARCHES = (("x-odd", 0, ODD, 8), ("y-odd", 1, ODD, 8), ("y-pow2", 1, (2, 4, 8), 3))
FMA_N = (3, 8)
GAP_N = (11, 12)
Y_TWINS = (("fma", 8), ("gap", 11))             # J-fma and J-gap once more on the y lines, at both sites


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> Case: the whole table (runs the searches; needs the oracle and the library's host calls)."""
    out = {}

    def add(name, width, n, site=SMALL, **kw):
        out[name] = Case(name, float(width), n, root=site.root, height=site.height, site=site.name, **kw)

    # J-r1 (J-neglx rides on the `up` member): odd lines in x with n = 8, power-of-two lines in y with n = 3,
    # at the small site (the reciprocal) and at the large one (the IEEE division)
    for site in (SMALL, LARGE):
        for tag, axis, cs, n in R1_SEARCHES:
            ts = r1_triples(site, "car", axis, cs)
            assert ts, f"no triple for {tag} at the {site.name} site"
            t = ts[0]
            for variant in ("up", "below", "above"):
                add(f"J-r1-{tag}-{site.name}-{t.first if variant == 'up' else variant}", getattr(t, variant), n, site,
                    target=t.slot, axis=axis, c=t.c, kind=f"r1-{t.first if variant == 'up' else variant}")
    tp = r1_triples(SMALL, "point", 0, (3, 5, 7, 9, 11, 13))
    assert tp, "no round-up triple for the point agent"
    for variant in ("up", "below", "above"):
        add(f"J-r1-point-{variant}", getattr(tp[0], variant), 1, agent="point", target=tp[0].slot, c=tp[0].c,
            kind=f"r1-{variant}")
    # J-minus1
    for axis in (0, 1):
        p = minus_one(axis)
        for variant, w in (("at", F32(p.width)), ("in", up(p.width)), ("out", down(p.width))):
            add(f"J-minus1-{'xy'[axis]}-{variant}", w, 1, CORNER, target=p.slot, axis=axis, c=0, kind=f"minus1-{variant}")
    # J-fma and J-gap at both sites
    for site in (SMALL, LARGE):
        for n in FMA_N:
            ps = fma_cases(site, n)
            assert ps, f"no contraction case for n = {n} at the {site.name} site"
            add(f"J-fma-n{n}-{site.name}", ps[0].width, n, site, target=ps[0].slot, axis=ps[0].axis, c=ps[0].c, kind="fma")
        for n in GAP_N:
            ps = gap_cases(SMALL_WIDE if site is SMALL else LARGE_WIDE, n)
            assert ps, f"no R2 gap child for n = {n} at the {site.name} site"
            add(f"J-gap-n{n}-{site.name}", ps[0].width, n, site, target=ps[0].slot, axis=ps[0].axis, c=ps[0].c, kind="gap")
    for site in (SMALL, LARGE):
        for kind, n in Y_TWINS:
            wide = SMALL_WIDE if site is SMALL else LARGE_WIDE
            ps = fma_cases(site, n, axis=1) if kind == "fma" else gap_cases(wide, n, axis=1)
            assert ps, f"no {kind} case in y for n = {n} at the {site.name} site"
            add(f"J-{kind}-y-n{n}-{site.name}", ps[0].width, n, site, target=ps[0].slot, axis=1, c=ps[0].c, kind=kind)
    # J-conc
    for n in (4, 12):
        for cov in (False, True):
            out[f"J-conc-n{n}-{'covered' if cov else 'free'}"] = Case(
                f"J-conc-n{n}-{'covered' if cov else 'free'}", 4000.0, n, root=CONC_ROOT, covering=cov, slots=65536,
                iterations=2, height=4000.0, kind="conc", site="conc")
    # two available cells: the root one unit under an R1 line, so some children cross it, and the score of
    # iterations 2 and 3 carries counts past 2^15 through 1 + R1^2 beside another cell's (s / s = 1 hides it above)
    out["J-conc-n4-two-cells"] = Case("J-conc-n4-two-cells", 4000.0, 4, root=CONC_LINE_ROOT, slots=65536, iterations=3,
                                      height=4000.0, kind="conc2", site="conc")
    return out


def _case_ids() -> tuple:
    ids = []
    for site in ("small", "large"):
        ids += [f"J-r1-x-odd-{site}-{v}" for v in ("up", "below", "above")]
        ids += [f"J-r1-y-odd-{site}-{v}" for v in ("up", "below", "above")]
        ids += [f"J-r1-y-pow2-{site}-{v}" for v in ("on", "below", "above")]
    ids += [f"J-r1-point-{v}" for v in ("up", "below", "above")]
    ids += [f"J-minus1-{a}-{v}" for a in "xy" for v in ("at", "in", "out")]
    for site in ("small", "large"):
        ids += [f"J-fma-n{n}-{site}" for n in FMA_N] + [f"J-gap-n{n}-{site}" for n in GAP_N]
    ids += [f"J-{kind}-y-n{n}-{site}" for site in ("small", "large") for kind, n in Y_TWINS]
    ids += [f"J-conc-n{n}-{v}" for n in (4, 12) for v in ("free", "covered")] + ["J-conc-n4-two-cells"]
    return tuple(ids)


CASE_IDS = _case_ids()      # the names of cases(), known without running the searches


# ---------------------------------------------------------------- J-accept and the batch entry
def expand_inputs(case: Case):
    """(parents (S, 7), rng (S, 6)) of iteration 1 as sbmp_expand_batch takes them."""
    o = make_oracle(scenario(case), plan=False)
    rng = o.rng()[:case.slots].copy()
    parents = np.tile(np.array(case.root + (0.0, 0.0, 0.0), dtype=np.float32), (case.slots, 1))
    return parents, rng


def check_expand(case: Case, got: dict, rng_before, R1Score, R2Avail, m: Model = Model()):
    """One expand_batch result against the model, child by child."""
    ch = got["children"]
    x, y = ch[:, 0].copy(), ch[:, 1].copy()
    valid = valid_children(x, y, case.width, case.height, case.covering)
    r1, r2, _ = model_cells(m, x, y, case.width, case.n)
    u = accept_draw(rng_before, m.draws_before)[0]
    _, st3, st4 = accept_draw(rng_before)
    acc = m.accept(valid, r1, r2, u, np.asarray(R1Score, dtype=F32), np.asarray(R2Avail))
    assert np.array_equal(got["valid"].astype(bool), valid)
    assert np.array_equal(got["r1"], r1) and np.array_equal(got["r2"], r2)
    assert np.array_equal(got["accept"].astype(bool), acc), \
        f"accept differs at {np.nonzero(got['accept'].astype(bool) != acc)[0][:8]}"
    assert np.array_equal(got["rng"], np.where(valid[:, None], st4, st3))
    return Seen(len(x), x, y, valid, r1, r2, u, np.asarray(R1Score, dtype=F32), acc)


# ---------------------------------------------------------------- J-root
@functools.lru_cache(maxsize=None)
def root_case() -> Case:
    """A root whose x is rounded up onto a cell line by the float division: seeded roots, the first hit."""
    rng = np.random.default_rng(99)
    for _ in range(200):
        x = F32(rng.uniform(6.0, 14.0))
        for c in (7, 11, 13):
            for W, hit in round_up_widths(np.array([x]), c):
                if hit[0] and SMALL.wmin <= W[0] <= SMALL.wmax and exact_quotient(x, W[0]) < c:
                    return Case("J-root", float(W[0]), 8, root=(float(x), 7.1, 0.7, 3.0), iterations=1, c=c, kind="root")
    raise AssertionError("no round-up root")


# ---------------------------------------------------------------- altered models (power tests)
def _floor_cell(q, count):
    with np.errstate(invalid="ignore"):
        t = np.floor(q)
        ok = np.isfinite(q) & (t >= 0) & (t < count)
    return np.where(ok, t, -1).astype(np.int64)


def _ge_minus_one_cell(q, count):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(q) & (q >= -1) & (q < count)
        return np.where(ok, np.maximum(np.trunc(q), 0), -1).astype(np.int64)


def _strict_accept(valid, r1, r2, u, R1Score, R2Avail_before):
    ok = valid & (r2 >= 0)
    return ok & ((u < R1Score[np.where(ok, r1, 0)]) | (R2Avail_before[np.where(ok, r2, 0)] == 0))


def _index_order_sum(s):
    total = F32(0)
    for v in np.asarray(s, dtype=F32):
        total = F32(total + v)
    return total


def _real_quotient(v, size):
    """The quotient to 53 bits: no float32 rounding onto a cell line."""
    return np.asarray(v, dtype=F64) / F64(size)


ALTERED = {
    "floor": Model(to_cell=staticmethod(_floor_cell)),
    "real-quotient": Model(quotient=staticmethod(_real_quotient)),
    "unfused-lx": Model(local=staticmethod(unfused_local)),
    "ge-minus-one": Model(to_cell=staticmethod(_ge_minus_one_cell)),
    "strict-accept": Model(accept=staticmethod(_strict_accept)),
    "early-draw": Model(draws_before=CONTROL_DRAWS - 1),
    "index-order-sum": Model(total=staticmethod(_index_order_sum)),
    "gap-counted-in-R2": Model(count_gap_in_R2=True),
    "float-denominator": Model(wide=F32),
    "real-quotient-y": Model(y=Model(quotient=staticmethod(_real_quotient))),
    "unfused-ly": Model(y=Model(local=staticmethod(unfused_local))),
}

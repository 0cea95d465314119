"""Family I, "goal edges": the verdict that ends a plan, at equality and one ulp either side,
and which row wins when several children enter the goal radius in one iteration.

The reference's goal test (inGoalRegion, KGMT.cu:635-638) is sqrt(dx*dx + dy*dy) < r on a
row as updateG inserts it, and the lowest inserted row inside the radius ends the plan (D4).
The planner restates it in k_step (at accept time, before the child is a row, followed by a
lane / wave / block-word / scan reduction of "lowest flagged goal child" and the clamp
jGoal < nIns && jGoal < M - tsPrev), in the sharded k_step (lowest row of blocks, then a walk
over the row's rank words), in the three insertion paths of the two-launch form (insert_block,
insert_blocks, insert_records with an atomicMin), per member in k_step_batch, and in the
public headers behind sbmp_insert_batch.  The other families run with goalThreshold = 0; the
demo's 0.5 radius never puts a child within an ulp of it.  Here it is put on a child's float.

Construction (pass 0).  The goal influences nothing but where the run stops, so a run of the
same shape with goalThreshold = 0 gives every row any goal can ever see, bit for bit.  Pass 0
steps the oracle with expand_local / local_records / finish; the records sorted by slot are
that iteration's flagged children in row order (row = treeSizeBefore + j), those that
capacity keeps out of the tree included.  The slot gives the child's place in the kernels:

    wave = slot // 64, block = slot // 256, scan thread = block // 4, scan wave = block // 256,
    owning rank of a shard group of P = block % P, row of blocks = block // P.

The independent model (`model`) is the reference's own operation order in float32 numpy,
unfused: dx = x - gx, dy = y - gy, d2 = fl(fl(dx*dx) + fl(dy*dy)), sqrt(d2) < thr (numpy's
float32 sqrt is correctly rounded), over pass 0's rows in row order, restricted per iteration
to j < min(A, 32 min(A, M // 32)) (the updateG grid, D6) and row < M (D13).  From it follow
goalIndex, iterations, treeSize, the bits of costToGoal and the solution path without the
oracle's goal code.  tests/test_goal_scenarios_oracle.py holds the model against the oracle
and asserts that every case below reaches the edge it claims; tests/test_gpu_goal_scenarios.py
runs the HIP planner on the same table.

Cases (all found by seeded searches over pass 0, not written down as constants; the searches'
properties are asserted by the oracle-only module, so another seed or RNG fails there):

  I-verdict   a goal a small non-round offset from a target row, the threshold on the target's
              float32 distance d: `at` (thr = d, strict <: not in the goal), `in` (thr = up(d):
              the plan ends on exactly that row), `out` (thr = down(d): as `at`).  No other row
              of the target's iteration or before lies within up(d).  The target is one for which
              the fused d2 = fl(fma(dx, dx, fl(dy*dy))) has a different square root than the
              unfused one, and among those the one whose exact sqrt(d2) lies nearest a float32
              rounding midpoint (found: 1.6e-5 ulp from the midpoint for the iteration-1 target,
              2.3e-4 for the iteration-3 one, 2.7e-3 on the 262,400-slot shape; the oracle-only
              module prints them and asserts < 1e-2): an approximate square root, `<=` for `<`
              or a contracted multiply-add moves one of the three variants.  One target among
              iteration 1's children (one parent) and one in iteration 3 (many parents).
  I-lowest    discs of one common radius per shape with at least two flagged children of
              iteration 1 inside, one disc per relation between the lowest candidate (the
              winner) and another candidate: `lanes` (one wave), `waves` (one block), `blocks`
              (one scan thread), `threads` (one scan wave), and on the 262,144-slot shape
              (1,024 blocks, which also takes the nBlocks == kMaxStepBlocks store of sPfx)
              `scan-waves` with the winner in scan wave 0, 1 and 2, plus one disc whose winner
              is in scan wave 3 (its other candidate can only be in a later scan thread of the
              same scan wave: rows grow with the slot).
              For shard groups: `P3-row` (one row of blocks, winner on rank 1, another candidate
              on rank 2, rank 0 of that row holds flagged children: the `pre +=` walk of
              row_goal and the masked words past the group), `P2-row-r1` (winner on rank 1; the
              row of a group of 2 has no later rank, so the other candidate shares its block),
              `P2-row-r0r1` (winner on rank 0, another candidate on rank 1 of the same row: the
              walk must stop at the first word) and `P2-rows` (candidates in different rows).
  I-capacity  D6: no boxes, root (10, 10, 0.3, 1.0), M = 1000, fill rule: iteration 1 flags 999
              children, the updateG grid inserts 992, the tree ends full.  The goal on the child
              of row 992 (d = 0, threshold the smallest subnormal) is found; on would-be row
              993 it is not.  With fixGNewClear on and off.  D13: a shape whose last insert is cut
              by capacity.  The batch rules keep S <= M - tsPrev, so tsPrev + A passes M only
              through flags that survived the partial GNew clear (D6), whose children are
              inserted again on top of the batch.  The goal on the child at j = M - tsPrev - 1
              (`D13-last-row`) is found at row M - 1.  The child at j = M - tsPrev lies past the
              batch (record j has a slot >= j >= S), so it is such a re-inserted child and a
              lower row already holds its float: a goal on it cannot stay unfound, whatever the
              seed, and the case the clamp jGoal < M - tsPrev alone would decide does not exist.
              `D13-first-cut` puts the goal there all the same: the plan ends on the lower row,
              iterations before, which the model and the oracle give alike.
  I-last      the `in` case with numIterations on the target's iteration (the flush pass inserts
              the row) and one less (the child is never created).
  I-threshold 0, -0, -1 and NaN never find, +inf finds row 1 at iteration 1, the goal on the
              root's own float finds whatever child comes first (row 0 is never tested).

Plain numpy plus the CPU oracle (at call time, not at import); no GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from scenarios import Scenario, demo_boxes, make_oracle

F32 = np.float32
TINY = float(np.nextafter(F32(0), F32(1)))        # the smallest positive subnormal
NOWHERE = (100.0, 100.0)                          # a goal no child comes near


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def no_boxes() -> np.ndarray:
    return np.zeros((0, 4), dtype=np.float32)


@dataclass(frozen=True, eq=False)
class Shape:
    name: str
    kw: dict                               # planner kwargs over DEMO + BASE (tests/scenarios.py)
    passes: int                            # numIterations of pass 0 and of every run not cut shorter
    boxes: object = demo_boxes
    initial: tuple = (5.0, 5.0, 0.0, 0.0)
    seed: int = 5
    radius: float = 0.0                    # the common radius of the shape's I-lowest discs

    def __str__(self):
        return self.name


# tests/scenarios.py's BASE scenario: 16,384 slots = 64 blocks = 16 scan threads
S16 = Shape("16k", {}, 4, radius=float(F32(0.0021)))
# 262,144 slots = 1,024 blocks = kMaxStepBlocks: four scan waves
BIG = Shape("262k", dict(samplesPerIteration=262144, maxTreeSize=1 << 20), 2, radius=float(F32(0.00063)))
# 262,400 slots = 1,025 blocks: the smallest shape past kMaxStepBlocks, so the planner takes the
# two-launch form and k_finish groups the blocks (finish_insert_groups: 264 insert workgroups of
# up to 4 blocks each, insert_blocks); up to 1,024 blocks every block has its own (insert_block)
GROUPED = Shape("262k4", dict(samplesPerIteration=262400, maxTreeSize=1 << 20), 1, radius=float(F32(0.00063)))
D6 = Shape("D6", dict(maxTreeSize=1000), 4, boxes=no_boxes, initial=(10.0, 10.0, 0.3, 1.0))
D6_PARTIAL = Shape("D6-partial-clear", dict(maxTreeSize=1000, fixGNewClear=False), 4, boxes=no_boxes,
                   initial=(10.0, 10.0, 0.3, 1.0))
# D13: the reference batch rule with the reference's partial GNew clear and n = 1.  Few children are
# accepted, so 32 A stays below the batch and flags past it survive (D6); their children are inserted
# again in every later iteration, on top of the new batch, and in the last one tsPrev + A passes M.
# Seed 305 is the one of 1 .. 399 (M = 700, 1000, 1500; n = 1, 2, 3) whose last row M - 1 takes a
# child of that iteration's own batch: in all others it is a re-inserted child, which lies on a
# lower row's float already.
D13 = Shape("D13", dict(maxTreeSize=1000, samplesPerIteration=4096, batchRule="reference", fixGNewClear=False), 200,
            seed=305)
SHAPES = (S16, BIG, GROUPED, D6, D6_PARTIAL, D13)


def scenario(shape: Shape, goal, thr: float, limit=None, env=None, local_group: int = 0) -> Scenario:
    kw = dict(shape.kw, goalThreshold=float(thr), numIterations=shape.passes if limit is None else int(limit))
    return Scenario(name=shape.name, family="I", targets="goal edges", kw=kw, boxes=shape.boxes,
                    initial=shape.initial, goal=(float(goal[0]), float(goal[1])), seed=shape.seed,
                    env=dict(env or {}), local_group=local_group)


# ---------------------------------------------------------------- pass 0
@dataclass(frozen=True, eq=False)
class Iteration:
    ts: int                 # treeSizeBefore
    slots: np.ndarray       # the flagged children in slot order: child j would be row ts + j
    xy: np.ndarray          # (A, 2) float32
    nIns: int               # min(A, 32 min(A, M // 32)): what the updateG grid inserts
    inserted: np.ndarray    # j < nIns and ts + j < M

    @property
    def A(self) -> int:
        return len(self.slots)


@dataclass(frozen=True, eq=False)
class Pass0:
    M: int
    logs: np.ndarray        # the oracle's iteration log of pass 0
    iters: tuple            # Iteration per iteration, from 1
    row: np.ndarray         # every inserted row past the root, ascending, with its
    it: np.ndarray          # iteration,
    slot: np.ndarray        # slot,
    x: np.ndarray           # and position (float32)
    y: np.ndarray
    samples: np.ndarray     # pass 0's tree
    parents: np.ndarray
    costs: np.ndarray
    end: tuple              # (iterations, treeSize) at pass 0's own end


@functools.lru_cache(maxsize=None)
def pass0(shape: Shape) -> Pass0:
    o = make_oracle(scenario(shape, NOWHERE, 0.0), plan=False)
    M = o.M
    iters = []
    while o.expand_local() >= 0:
        rec = o.local_records()
        rec = rec[np.argsort(rec["slot"], kind="stable")]
        ts = int(o.info()["treeSize"])
        o.finish(rec, o.local_deltas())
        A = len(rec)
        nIns = min(A, 32 * min(A, M // 32))
        j = np.arange(A)
        iters.append(Iteration(ts, rec["slot"].astype(np.int64), np.ascontiguousarray(rec["sample"][:, :2]), nIns,
                               (j < nIns) & (ts + j < M)))
    logs = o.iter_logs()
    assert len(logs) == len(iters) and [i.ts for i in iters] == logs[:, 1].tolist()
    assert [i.A for i in iters] == logs[:, 6].tolist()
    samples, parents, costs = o.tree()
    info = o.info()
    assert info["goalIdx"] == -1

    def flat(f):
        return np.concatenate([f(k + 1, i)[i.inserted] for k, i in enumerate(iters)])
    p = Pass0(M, logs, tuple(iters),
              row=flat(lambda k, i: i.ts + np.arange(i.A)), it=flat(lambda k, i: np.full(i.A, k)),
              slot=flat(lambda k, i: i.slots), x=flat(lambda k, i: i.xy[:, 0]), y=flat(lambda k, i: i.xy[:, 1]),
              samples=samples, parents=parents, costs=costs, end=(info["iterations"], info["treeSize"]))
    for a in (p.row, p.it, p.slot, p.x, p.y, samples, parents, costs, logs):
        a.setflags(write=False)
    return p


# ---------------------------------------------------------------- the independent model
def distance(x, y, goal):
    """inGoalRegion's left-hand side in the reference's operation order, float32, unfused."""
    dx = np.asarray(x, dtype=F32) - F32(goal[0])
    dy = np.asarray(y, dtype=F32) - F32(goal[1])
    xx = (dx * dx).astype(F32)
    yy = (dy * dy).astype(F32)
    return np.sqrt((xx + yy).astype(F32), dtype=F32)


@dataclass(frozen=True)
class Expect:
    goalIndex: int
    iterations: int
    treeSize: int
    cost_bits: int          # costToGoal's bits (0.0 without a goal)
    path: tuple             # rows root .. goalIndex, () without a goal


def chain(p: Pass0, row: int) -> tuple:
    rows = [int(row)]
    while p.parents[rows[-1]] >= 0:
        rows.append(int(p.parents[rows[-1]]))
    return tuple(rows[::-1])


def model(shape: Shape, goal, thr, limit=None) -> Expect:
    p = pass0(shape)
    limit = shape.passes if limit is None else int(limit)
    with np.errstate(invalid="ignore"):
        hit = (distance(p.x, p.y, goal) < F32(thr)) & (p.it <= limit)
    idx = np.nonzero(hit)[0]
    if len(idx):
        k = int(idx[0])     # rows ascend: the lowest inserted row inside the radius (D4)
        row, it = int(p.row[k]), int(p.it[k])
        return Expect(row, it, int(p.logs[it - 1, 7]), int(p.costs[row:row + 1].view(np.uint32)[0]), chain(p, row))
    its = min(limit, p.end[0])
    return Expect(-1, its, int(p.logs[its - 1, 7]) if its else 1, 0, ())


# ---------------------------------------------------------------- where a slot sits in the kernels
def units(slot: int, P: int = 1) -> dict:
    block = int(slot) // 256
    return dict(lane=int(slot) % 64, wave=int(slot) // 64, block=block, thread=block // 4, scan_wave=block // 256,
                rank=block % P, block_row=block // P)


def relation(a: int, b: int) -> str:
    """The first reduction level at which slots a and b part."""
    ua, ub = units(a), units(b)
    if ua["wave"] == ub["wave"]:
        return "lanes"
    if ua["block"] == ub["block"]:
        return "waves"
    if ua["thread"] == ub["thread"]:
        return "blocks"
    if ua["scan_wave"] == ub["scan_wave"]:
        return "threads"
    return "scan-waves"


# ---------------------------------------------------------------- I-verdict
def fl32(q: Fraction) -> np.float32:
    """q rounded to float32, to nearest and ties to even, exactly."""
    f = F32(float(q))
    return min((down(f), f, up(f)), key=lambda c: (abs(Fraction(float(c)) - q), int(c.view(np.uint32)) & 1))


def fused_distance(x, y, goal) -> np.float32:
    """sqrt of d2 = fl(fma(dx, dx, fl(dy*dy))), the multiply-add rounded once (exact arithmetic)."""
    dx, dy = F32(x) - F32(goal[0]), F32(y) - F32(goal[1])
    yy = F32(dy * dy)
    return np.sqrt(fl32(Fraction(float(dx)) ** 2 + Fraction(float(yy))), dtype=F32)


def midpoint_gap(x, y, goal) -> float:
    """How far, in ulps of the result, the exact sqrt(d2) lies from the nearer rounding midpoint."""
    dx, dy = F32(x) - F32(goal[0]), F32(y) - F32(goal[1])
    d2 = F32(F32(dx * dx) + F32(dy * dy))
    d = np.sqrt(d2, dtype=F32)
    return 0.5 - abs(float(np.sqrt(np.float64(d2))) - float(d)) / float(np.spacing(d))


@dataclass(frozen=True)
class Verdict:
    shape: Shape
    row: int
    it: int
    slot: int
    goal: tuple
    d: float                # the target's float32 distance

    def thr(self, variant: str) -> float:
        return float({"at": F32(self.d), "in": up(self.d), "out": down(self.d)}[variant])


@functools.lru_cache(maxsize=None)
def verdict(shape: Shape, it: int) -> Verdict:
    p = pass0(shape)
    rng = np.random.default_rng(7000 + it)
    seen = np.nonzero(p.it <= it)[0]
    K = 200000
    t = rng.choice(np.nonzero(p.it == it)[0], K)
    ang, rad = rng.uniform(0.0, 2.0 * np.pi, K), rng.uniform(0.4e-3, 2.5e-3, K)
    gx = (p.x[t] + (rad * np.cos(ang)).astype(F32)).astype(F32)
    gy = (p.y[t] + (rad * np.sin(ang)).astype(F32)).astype(F32)
    dx, dy = p.x[t] - gx, p.y[t] - gy
    yy = (dy * dy).astype(F32)
    d2 = ((dx * dx).astype(F32) + yy).astype(F32)
    d = np.sqrt(d2, dtype=F32)
    # the fused form in float64 (a 48-bit product plus a float32): exact but for rare double roundings,
    # which the exact arithmetic of fused_distance settles for the chosen candidate
    fused = np.sqrt((dx.astype(np.float64) ** 2 + yy.astype(np.float64)).astype(F32), dtype=F32)
    cand = np.nonzero((fused != d) & (d > 0))[0]
    gap = 0.5 - np.abs(np.sqrt(d2[cand].astype(np.float64)) - d[cand].astype(np.float64)) / np.spacing(d[cand])
    for c in cand[np.argsort(gap, kind="stable")]:
        goal = (float(gx[c]), float(gy[c]))
        others = seen[seen != t[c]]
        if (distance(p.x[others], p.y[others], goal) > up(d[c])).all() and fused_distance(p.x[t[c]], p.y[t[c]], goal) != d[c]:
            return Verdict(shape, int(p.row[t[c]]), it, int(p.slot[t[c]]), goal, float(d[c]))
    raise AssertionError(f"{shape} iteration {it}: no isolated FMA-sensitive target")


VARIANTS = ("at", "in", "out")
VERDICTS = ((S16, 1), (S16, 3), (GROUPED, 1))     # (shape, the target's iteration)


# ---------------------------------------------------------------- I-lowest
@dataclass(frozen=True)
class Disc:
    shape: Shape
    name: str
    goal: tuple
    rows: tuple             # the candidates' rows, ascending: rows[0] wins
    slots: tuple

    @property
    def thr(self) -> float:
        return self.shape.radius


# name -> (P, predicate over the winner's slot and the other candidates' slots)
DISC_KINDS = {
    "lanes": lambda w, o: any(relation(w, s) == "lanes" for s in o),
    "waves": lambda w, o: any(relation(w, s) == "waves" for s in o),
    "blocks": lambda w, o: any(relation(w, s) == "blocks" for s in o),
    "threads": lambda w, o: any(relation(w, s) == "threads" for s in o),
    "P3-row": lambda w, o: units(w, 3)["rank"] == 1 and any(
        units(s, 3)["block_row"] == units(w, 3)["block_row"] and units(s, 3)["rank"] == 2 for s in o),
    "P2-row-r1": lambda w, o: units(w, 2)["rank"] == 1 and any(units(s)["block"] == units(w)["block"] for s in o),
    "P2-row-r0r1": lambda w, o: units(w, 2)["rank"] == 0 and any(
        units(s, 2)["block_row"] == units(w, 2)["block_row"] and units(s, 2)["rank"] == 1 for s in o),
    "P2-rows": lambda w, o: any(units(s, 2)["block_row"] != units(w, 2)["block_row"] for s in o),
}
BIG_KINDS = {
    "scan-waves-w0": lambda w, o: units(w)["scan_wave"] == 0 and any(relation(w, s) == "scan-waves" for s in o),
    "scan-waves-w1": lambda w, o: units(w)["scan_wave"] == 1 and any(relation(w, s) == "scan-waves" for s in o),
    "scan-waves-w2": lambda w, o: units(w)["scan_wave"] == 2 and any(relation(w, s) == "scan-waves" for s in o),
    "threads-w3": lambda w, o: units(w)["scan_wave"] == 3 and any(relation(w, s) == "threads" for s in o),
}
GROUPED_KINDS = {
    # candidates in different blocks, and one with a candidate in block 1024, the one block past
    # kMaxStepBlocks (insert workgroup 1024 - 3 * 264 = 232 takes blocks 232, 496, 760 and 1024)
    "other-block": lambda w, o: any(units(s)["block"] != units(w)["block"] for s in o),
    "last-block": lambda w, o: units(w)["block"] < 1024 and any(units(s)["block"] == 1024 for s in o),
}
KINDS = {S16: DISC_KINDS, BIG: BIG_KINDS, GROUPED: GROUPED_KINDS}


@functools.lru_cache(maxsize=None)
def discs(shape: Shape) -> dict:
    """name -> Disc over iteration 1's children: seeded random centres, the first that fits each kind."""
    p = pass0(shape)
    r = F32(shape.radius)
    first = np.nonzero(p.it == 1)[0]
    order = first[np.argsort(p.x[first], kind="stable")]
    xs = p.x[order]
    rng = np.random.default_rng(4242)
    kinds = KINDS[shape]
    found = {}
    for _ in range(60000):
        c = int(first[rng.integers(len(first))])
        gx = F32(p.x[c] + F32(rng.uniform(-0.6, 0.6) * float(r)))
        gy = F32(p.y[c] + F32(rng.uniform(-0.6, 0.6) * float(r)))
        near = order[np.searchsorted(xs, gx - r - F32(1e-4)):np.searchsorted(xs, gx + r + F32(1e-4))]
        inside = np.sort(near[distance(p.x[near], p.y[near], (gx, gy)) < r])
        if not 2 <= len(inside) <= 6:   # a handful, so that a case stays readable
            continue
        slots = [int(s) for s in p.slot[inside]]
        for name, fits in kinds.items():
            if name not in found and fits(slots[0], slots[1:]):
                found[name] = Disc(shape, name, (float(gx), float(gy)), tuple(int(v) for v in p.row[inside]), tuple(slots))
        if len(found) == len(kinds):
            return found
    raise AssertionError(f"{shape}: no disc for {sorted(set(kinds) - set(found))}")


def disc_params():
    return [(shape, name) for shape in (S16, BIG, GROUPED) for name in KINDS[shape]]


# ---------------------------------------------------------------- I-capacity
@dataclass(frozen=True)
class Capacity:
    shape: Shape
    name: str
    it: int                 # the iteration whose insert is clamped
    j: int                  # the child the goal sits on
    goal: tuple
    inserted: bool          # whether the clamps let child j become a row
    row: object             # the row that ends the plan: ts + j, -1 for none, None for "a lower row" (D13)
    thr: float = TINY


def cut_iteration(shape: Shape) -> int:
    """The iteration of pass 0 whose insert passes M (D13)."""
    p = pass0(shape)
    cut = [k + 1 for k, i in enumerate(p.iters) if i.ts < p.M < i.ts + i.A]
    assert len(cut) == 1, cut
    return cut[0]


def capacity_cases() -> list:
    out = []
    for shape in (D6, D6_PARTIAL):      # the updateG grid: rows 1 .. 992 are written, 993 .. 999 are not
        i = pass0(shape).iters[0]
        for j, ins in ((i.nIns - 1, True), (i.nIns, False)):
            out.append(Capacity(shape, f"{shape.name}-row{i.ts + j}", 1, j, tuple(float(v) for v in i.xy[j]), ins,
                                i.ts + j if ins else -1))
    it = cut_iteration(D13)
    i = pass0(D13).iters[it - 1]
    j = pass0(D13).M - i.ts - 1         # the last child capacity lets in, and the first it keeps out
    out.append(Capacity(D13, "D13-last-row", it, j, tuple(float(v) for v in i.xy[j]), True, i.ts + j))
    out.append(Capacity(D13, "D13-first-cut", it, j + 1, tuple(float(v) for v in i.xy[j + 1]), False, None))
    return out


CAPACITY_IDS = ("D6-row992", "D6-row993", "D6-partial-clear-row992", "D6-partial-clear-row993", "D13-last-row",
                "D13-first-cut")


# ---------------------------------------------------------------- I-threshold
def threshold_cases() -> list:
    """(id, goal, threshold) on the 16k shape; the goal of the first four is the verdict target's."""
    g = verdict(S16, 1).goal
    root = S16.initial[:2]
    return [("zero", g, 0.0), ("minus-zero", g, -0.0), ("minus-one", g, -1.0), ("nan", g, float("nan")),
            ("inf", g, float("inf")), ("root-0.05", root, 0.05), ("root-subnormal", root, TINY)]


THRESHOLD_IDS = ("zero", "minus-zero", "minus-one", "nan", "inf", "root-0.05", "root-subnormal")


# ---------------------------------------------------------------- iteration 1 as sbmp_insert_batch's input
def insert_inputs(shape: Shape):
    """(gnew, unexplored, uParent, samples, parent, costs, treeSize) before iteration 1's insert."""
    p = pass0(shape)
    o = make_oracle(scenario(shape, NOWHERE, 0.0), plan=False)
    assert o.step()
    S = int(p.logs[0, 5])
    u, up_ = o.unexplored()
    gnew = np.zeros(S, dtype=np.uint8)
    gnew[p.iters[0].slots] = 1
    samples = np.zeros((p.M, 7), dtype=np.float32)
    samples[0] = p.samples[0]
    parent = np.full(p.M, -1, dtype=np.int32)
    return gnew, u[:S].copy(), up_[:S].copy(), samples, parent, np.zeros(p.M, dtype=np.float32), 1


def insert_cases() -> list:
    """(id, shape, goal, threshold) for sbmp_insert_batch: the I-verdict triple and the D6 pair."""
    v = verdict(S16, 1)
    out = [(f"verdict-{k}", S16, v.goal, v.thr(k)) for k in VARIANTS]
    out += [(c.name, c.shape, c.goal, c.thr) for c in capacity_cases() if c.shape is D6]
    return out


INSERT_IDS = ("verdict-at", "verdict-in", "verdict-out", "D6-row992", "D6-row993")

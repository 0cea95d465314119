"""Sequence table for the handle-reuse parity tests: many plans on one planner handle.

A replanning loop calls begin() / plan() again and again on one handle, each call with
another start, goal, seed and obstacle list.  A sequence here is a handle configuration
plus an ordered list of plans; the state one plan leaves behind (tree rows, used slots,
ctrl blocks, region tables, the grown obstacle buffers, the host-side form flags) is what
its successor must not see.  tests/test_reuse_scenarios_oracle.py proves on the CPU oracle
alone that every predecessor leaves something its successor is sensitive to (the `claims`
of each adjacent pair); tests/test_gpu_reuse_scenarios.py drives the sequences on one HIP
handle each and compares every plan with a fresh oracle run and a fresh handle's digest.

Plain numpy: no GPU and no oracle at import.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from conftest import DEMO
from scenarios import EXTRA_KEYS, ROOT_STATE, demo_boxes, demo_plus, make_oracle, random_boxes

FAR = (40.0, 40.0)        # outside the 20 x 20 workspace: never reached
LDS_ROOT = (15.0, 15.0, 1.0, 0.5)
NAN = float("nan")

LOG = {n: i for i, n in enumerate(("itr", "treeSizeBefore", "nG", "k", "nExp", "S", "A", "treeSizeAfter", "goalIdx"))}

# Conditions a pair (P, Q) of consecutive plans may claim.  '>' reads "P's exceeds Q's".
CONDITIONS = ("rows>", "rows<", "slots>", "slots<", "iterations>", "iterations<", "cells>", "cells<", "form", "parity")


def no_boxes() -> np.ndarray:
    return np.zeros((0, 4), dtype=np.float32)


def lds_600() -> np.ndarray:
    return random_boxes(600, 20.0, 20.0, 7, 0.3, 0.8, root=LDS_ROOT)


def grid_3000() -> np.ndarray:
    return random_boxes(3000, 20.0, 20.0, 11, 0.08, 0.5)


def grid_2100() -> np.ndarray:
    return random_boxes(2100, 20.0, 20.0, 13, 0.15, 0.5)


def nan_list() -> np.ndarray:
    return demo_plus((NAN, NAN, NAN, NAN))


def c5_2048() -> np.ndarray:
    """The first 2,048 boxes of the 10,000-box field (tests/test_gpu_headline.py's LDS list)."""
    from test_gpu_headline import _c5_obstacles
    return _c5_obstacles()[:2048].copy()


@dataclass(frozen=True)
class Plan:
    tag: str
    seed: int
    goal: tuple = FAR
    boxes: Callable[[], np.ndarray] = demo_boxes
    initial: tuple = ROOT_STATE            # (x, y, theta, v)
    obstacle_form: str = "registers"       # path_info() after this plan's begin()
    nan: bool = False                      # the list holds a NaN (obsNaN)
    # how the plan is driven:
    #   "plan"     plan()
    #   "step"     begin(), the whole state compared with a begun oracle, then step() to the end
    #   "enqueue"  begin(), the same comparison, enqueue(iterations), no sync: abandoned, the next begin() meets it in flight
    #   "abandon"  begin(), step(iterations), tree() read: abandoned mid-plan
    drive: str = "plan"
    iterations: int = 0                    # of an abandoned plan
    # calls round the plan that the GPU test makes (tests/test_gpu_reuse_scenarios.py):
    #   "passes"        after: recheck(LDS-600's boxes), query_goals(alive=True), trace(), solution_paths()
    #   "alive_raises"  between begin() and the first step: query_goals(alive=True) raises SbmpError
    #   "recheck"       after: recheck(LDS-600's boxes) equals tests/tree_recheck_model.py on the new tree
    #   "clobber"       between begin() and the first step: the caller's obstacle array is overwritten and freed
    hooks: tuple = ()

    @property
    def abandoned(self) -> bool:
        return self.drive in ("enqueue", "abandon")

    def obstacles(self) -> np.ndarray:
        return np.ascontiguousarray(self.boxes(), dtype=np.float32).reshape(-1, 4)

    def initial7(self):
        return tuple(self.initial) + (0.0, 0.0, 0.0)

    def goal7(self):
        return tuple(self.goal) + (0.0,) * 5


# The building blocks (each measured on the CPU oracle at the DEMO configuration; the
# figures are asserted by tests/test_reuse_scenarios_oracle.py's MEASURED table).
LONG_FREE = Plan("LONG-free", seed=5, boxes=no_boxes)
LONG_DEMO = Plan("LONG-demo", seed=5)
# seed 3, not 6: one of its 32 children is invalid and is rejected, so even this one-iteration plan has both kinds
SHORT = Plan("SHORT", seed=3, goal=(6.5, 5.0))
DEMO_PLAN = Plan("DEMO", seed=1, goal=(2.0, 18.0))
LDS_600 = Plan("LDS-600", seed=7, boxes=lds_600, initial=LDS_ROOT, obstacle_form="lds")
GRID_3000 = Plan("GRID-3000", seed=8, boxes=grid_3000, obstacle_form="grid")
GRID_2100 = Plan("GRID-2100", seed=9, boxes=grid_2100, obstacle_form="grid")
NAN_PLAN = Plan("NaN-list", seed=5, boxes=nan_list, nan=True)
TINY = Plan("TINY", seed=5)
TINY_SHORT = Plan("TINY-short", seed=3, goal=(6.5, 5.0))
TINY_6 = Plan("TINY-seed6", seed=6)


def _with(p: Plan, **changes) -> Plan:
    f = {k: getattr(p, k) for k in p.__dataclass_fields__}
    f.update(changes)
    return Plan(**f)


@dataclass(frozen=True)
class Sequence:
    name: str
    targets: str
    plans: tuple
    claims: tuple                                    # one tuple of CONDITIONS per adjacent pair
    kw: dict = field(default_factory=dict)           # planner kwargs over DEMO
    env: dict = field(default_factory=dict)          # SBMP_STEP, set before construction
    local_group: int = 0
    step_forms: Optional[tuple] = None               # path_info()["form"] per plan; None: by env
    stalls: tuple = ()                               # tags of plans whose every child is invalid (no spread)

    def config(self):
        """(cfg, extra): the KGMT positional configuration and its keyword extras."""
        full = dict(DEMO)
        full.update(self.kw)
        extra = {k: full.pop(k) for k in EXTRA_KEYS if k in full}
        return full, extra

    def step_form(self, i: int) -> str:
        if self.step_forms is not None:
            return self.step_forms[i]
        return "two-launch" if self.env.get("SBMP_STEP") == "0" else "k_step"


class _Run:
    """One plan on one sequence's configuration, in the shape scenarios.make_oracle takes."""

    def __init__(self, seq: Sequence, plan: Plan):
        self.seq, self.plan, self.seed = seq, plan, plan.seed
        self.config, self.initial7, self.goal7, self.obstacles = seq.config, plan.initial7, plan.goal7, plan.obstacles


_ORACLES = {}
CACHE_ROWS = 1 << 20    # an oracle of more rows (S11's 2^24) is not kept


def oracle_run(seq: Sequence, plan: Plan, threads: int = 8):
    """A fresh oracle run of `plan` alone on `seq`'s configuration: to its end, or through
    plan.iterations iterations for an abandoned plan.  Kept in memory (read only) per
    (configuration, plan); the two callers never change one."""
    cfg, extra = seq.config()
    key = (tuple(sorted(cfg.items())), tuple(sorted(extra.items())), plan.obstacles().tobytes(), plan.initial, plan.goal,
           plan.seed, plan.iterations if plan.abandoned else 0)
    if key in _ORACLES:
        return _ORACLES[key]
    o = make_oracle(_Run(seq, plan), threads=threads, plan=not plan.abandoned)
    for _ in range(plan.iterations if plan.abandoned else 0):
        if not o.step():
            break
    if cfg["maxTreeSize"] <= CACHE_ROWS:
        _ORACLES[key] = o
    return o


def oracle_begun(seq: Sequence, plan: Plan):
    """A fresh oracle after begin() of `plan` alone, no iteration run: the constructor state
    (zero tables, parents -1, R1Score 1.0), the root, the seeded RNG."""
    return make_oracle(_Run(seq, plan), threads=1, plan=False)


def _build() -> list:
    from test_gpu_headline import _bench_kw   # the benchmark's shape; that module needs no GPU at import
    Q = []

    def add(name, targets, plans, claims, **rest):
        assert len(claims) == len(plans) - 1, name
        Q.append(Sequence(name=name, targets=targets, plans=tuple(plans), claims=tuple(tuple(c) for c in claims), **rest))

    # ---- S1 long -> short -> long: the short plan sits on 29,969 stale rows, 23,712 used
    #      slots, 100 ctrl blocks and every R1 cell (its own 32 children touch 5); the third shows it left nothing
    #      (SHORT is stepped: its state is also compared right after begin(), the only moment
    #      at which the R1Score buffer of even iterations shows what begin() left in it)
    s1 = [LONG_FREE, _with(SHORT, drive="step"), LONG_DEMO]
    s1_claims = [("rows>", "slots>", "iterations>", "cells>", "form", "parity"),
                 ("rows<", "slots<", "iterations<", "cells<", "parity")]
    add("S1-long-short-long", "stale rows, slots, ctrl blocks and R1 cells under a one-iteration plan", s1, s1_claims)

    # ---- S2 every obstacle form on one handle: obs_ / gridStart_ / gridBoxes_ grow and then
    #      hold a shorter list; gridG, obsNaN and the LDS staging change under a live handle
    s2 = [DEMO_PLAN, LDS_600, GRID_3000, LONG_FREE, NAN_PLAN, SHORT, GRID_2100, DEMO_PLAN]
    s2_claims = [("rows<", "slots<", "iterations<", "form", "parity"), ("rows<", "slots<", "cells>", "form"),
                 ("rows<", "slots>", "cells>", "form"), ("rows>", "slots>", "cells>", "form"),
                 ("rows<", "iterations>", "cells<", "form", "parity"),
                 ("rows<", "slots<", "iterations<", "cells<", "form", "parity"),
                 ("rows>", "slots>", "iterations>", "cells>", "form", "parity")]
    add("S2-every-obstacle-form", "registers, lds, grid, none, NaN, registers, a shorter grid list, registers",
        s2, s2_claims, stalls=("NaN-list",))

    # ---- S3 an unsynced predecessor: begin() meets 3 (then 4) iterations still in flight;
    #      with 4 the exchange and publish buffers of both parities were the last written
    for n in (3, 4):
        add(f"S3-unsynced-{n}", f"begin() over {n} enqueued, unwaited iterations (k_step: the last one not inserted)",
            [_with(LONG_DEMO, drive="enqueue", iterations=n), _with(DEMO_PLAN, drive="step")],
            [("iterations<", "rows<", "slots<", "cells>") + (("parity",) if n == 4 else ())])

    #      the same over the grid index: begin() rebuilds the cell-start table and the box copies,
    #      from the host and outside the stream, under a predecessor that may still read them
    add("S3-unsynced-grid", "begin() with a shorter grid list over 3 unwaited iterations on the 3,000-box grid",
        [_with(GRID_3000, drive="enqueue", iterations=3), _with(GRID_2100, drive="step")],
        [("iterations<", "rows<", "slots<", "form")])

    # ---- S4 an abandoned predecessor
    add("S4-abandoned", "begin(); step(2); tree(); then other plans",
        [_with(LONG_DEMO, drive="abandon", iterations=2), SHORT, DEMO_PLAN],
        [("rows>", "slots>", "iterations>", "cells>"), ("rows<", "slots<", "iterations<", "cells<")])

    # ---- S5 after the grown-tree passes (their scratch, the alive mask, the re-check's own list)
    add("S5-after-tree-passes", "recheck / query_goals(alive) / trace / solution_paths before the next begin()",
        [_with(DEMO_PLAN, hooks=("passes",)), _with(SHORT, drive="step", hooks=("alive_raises", "recheck")), DEMO_PLAN],
        [("rows>", "slots>", "iterations>", "cells>"), ("rows<", "slots<", "iterations<", "cells<")])

    # ---- S6 the caller's obstacle array is the caller's: begin() documents a private copy
    add("S6-callers-array", "the caller overwrites and frees its obstacle array after begin()",
        [LONG_FREE, _with(DEMO_PLAN, drive="step", hooks=("clobber",))], [("rows>", "slots>", "iterations>", "cells>", "form", "parity")])

    # ---- S7 the two-launch handle
    add("S7-two-launch-S1", "S1 on the two-launch form (k_expand + k_finish)", s1, s1_claims, env={"SBMP_STEP": "0"})
    for n in (3, 4):
        add(f"S7-two-launch-S3-{n}", f"S3 ({n} unwaited iterations) on the two-launch form",
            [_with(LONG_DEMO, drive="enqueue", iterations=n), _with(DEMO_PLAN, drive="step")],
            [("iterations<", "rows<", "slots<", "cells>") + (("parity",) if n == 4 else ())], env={"SBMP_STEP": "0"})

    # ---- S8 point agent (theta and v of the roots are ignored)
    add("S8-point", "S1's plans with the point agent", s1,
        [("rows>", "slots>", "iterations>", "cells>", "form"), ("rows<", "slots<", "iterations<", "cells<")],
        kw=dict(agent="point"))

    # ---- S9 local shard groups: begin() does not clear stepCnt / stepDelta / stepR2New on a
    #      sharded rank, and each owner keeps its own GNew words
    for P in (2, 3):
        add(f"S9-group{P}-S1", f"S1 on {P} local ranks", s1, s1_claims, local_group=P)
        add(f"S9-group{P}-S2", f"S2's first four plans on {P} local ranks", s2[:4], s2_claims[:3], local_group=P)
        for n in (3, 4):   # 4: xSend / xSendOdd and the group's sum buffer of both parities were the last written
            add(f"S9-group{P}-S3-{n}", f"S3 ({n} unwaited iterations) on {P} local ranks",
                [_with(LONG_DEMO, drive="enqueue", iterations=n), _with(DEMO_PLAN, drive="step")],
                [("iterations<", "rows<", "slots<", "cells>") + (("parity",) if n == 4 else ())], local_group=P)

    # ---- S10 the 700-row handle: the k = 0 path and a full-tree ending as predecessors
    add("S10-tiny", "a 700-row handle: k = 0 iterations, then one iteration, then 50 again",
        [TINY, TINY_SHORT, TINY_6], [("rows>", "slots>", "iterations>", "cells>", "parity"),
                                     ("rows<", "slots<", "iterations<", "cells<", "parity")],
        kw=dict(maxTreeSize=700, numIterations=50))

    # ---- S11 the step form changes under the handle (the only large shape): c3 size, two
    #      iterations; 1,025 resident groups against a 2,048-box LDS list
    c3 = dict(seed=20240807, goal=(2.0, 18.0))
    add("S11-step-form-changes", "k_step, then the two-launch form for a 2,048-box LDS list, then k_step again",
        [Plan("C3-demo", **c3), Plan("C3-lds-2048", boxes=c5_2048, obstacle_form="lds", **c3), Plan("C3-demo", **c3)],
        [("form",), ("form",)], kw=_bench_kw(262144, 2), step_forms=("k_step", "two-launch", "k_step"))
    return Q


SEQUENCES = _build()
IDS = [s.name for s in SEQUENCES]
assert len(set(IDS)) == len(IDS)


# ---- S12 a batch: KGMTBatch(count, DEMO); every row is one plan() of the batch:
#      (boxes, obstacle form, per-member roots, goals, seeds)
BATCH_ROOTS = [ROOT_STATE, (5.5, 4.5, 0.3, 0.0), (4.5, 5.25, -1.0, 0.5)]
BATCH_GOAL = (2.0, 18.0)


@dataclass(frozen=True)
class BatchSequence:
    name: str
    count: int
    plans: tuple    # of (tag, boxes, obstacle form, roots, goals, seeds)
    claims: tuple   # per adjacent pair of rows: CONDITIONS that hold for every member

    def member_sequence(self) -> Sequence:
        """The members' configuration (DEMO), for oracle_run."""
        return Sequence(name=self.name, targets="", plans=(), claims=())

    def member_plan(self, row, i: int) -> Plan:
        tag, boxes, form, roots, goals, seeds = row
        return Plan(f"{tag}[{i}]", seed=seeds[i], goal=goals[i], boxes=boxes, initial=roots[i], obstacle_form=form)


def _batch() -> list:
    def row(tag, boxes, form, count, roots, seed0, goal=BATCH_GOAL):
        return (tag, boxes, form, tuple(roots[i % len(roots)] for i in range(count)), (goal,) * count,
                tuple(range(seed0, seed0 + count)))

    lds_roots = [LDS_ROOT, (15.5, 14.5, 0.3, 0.0), (14.5, 15.25, -1.0, 0.5)]
    return [
        BatchSequence("S12-batch3", 3, (row("demo", demo_boxes, "registers", 3, BATCH_ROOTS, 1),
                                        row("lds-600", lds_600, "lds", 3, lds_roots, 21, goal=FAR),
                                        row("grid-3000", grid_3000, "grid", 3, BATCH_ROOTS[::-1], 31, goal=FAR),
                                        row("demo-again", demo_boxes, "registers", 3, BATCH_ROOTS, 41)),
                      (("rows<", "iterations<", "form"), ("form",), ("rows>", "iterations>", "form"))),
        BatchSequence("S12-batch12", 12, (row("demo", demo_boxes, "registers", 12, BATCH_ROOTS, 1),
                                          row("lds-600", lds_600, "lds", 12, lds_roots, 21, goal=FAR)),
                      (("iterations<", "form"),)),
    ]


BATCHES = _batch()
BATCH_IDS = [b.name for b in BATCHES]

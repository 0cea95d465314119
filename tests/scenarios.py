"""Scenario table for the planner-level parity tests beyond the demo's square scene.

Every scenario aims at the edge of one shortcut of the hot loop (car_euler_fast,
car_schedule, wave_cull, car_theta_bounded, bins_k, the unmasked grid query).
tests/test_scenarios_oracle.py proves on the CPU oracle alone that a scenario
reaches its edge (its `cover` conditions); tests/test_gpu_scenarios.py compares
the HIP planner with the oracle bit for bit on the same table.

Family F's F-touching-root / F-touching-root-next test one box comparison at equality;
they are now one of a full set, family H ("verdict edges": every comparison and both
movable walls, in every obstacle form), which needs an oracle pass to build its boxes
and so has its own module, tests/edge_scenarios.py.

Plain numpy: no GPU and no oracle at import.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from conftest import DEMO, OBSTACLES_CSV

# The one small base every scenario derives from; none is larger in slots or iterations.
# With the demo boxes the frontier passes through 64 <= k < 256 with one or two parents
# per wave (car_schedule valid) and through k < 64 (no schedule, car_cull).
BASE = dict(samplesPerIteration=16384, batchRule="fill", fixGNewClear=True, n=1, maxTreeSize=200000,
            numIterations=12, goalThreshold=0.0)
BASE_SEED = 5
EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")

ROOT_STATE = (5.0, 5.0, 0.0, 0.0)
GOAL = (2.0, 18.0)

CW_LIMIT = 105615.0       # sincos_pred: Cody-Waite up to here, Payne-Hanek past it
BOUNDED_LIMIT = 100000.0  # car_theta_bounded: Cody-Waite alone below this bound


def demo_boxes() -> np.ndarray:
    return np.loadtxt(OBSTACLES_CSV, delimiter=",", dtype=np.float32).reshape(-1, 4)


# The three boxes test_edge_cases_bit_exact adds to the demo's five.
MORE_BOXES = np.array([[10, 12, 11, 13], [14, 3, 15, 4], [12, 15, 13, 16]], dtype=np.float32)


def demo_prefix(count: int) -> np.ndarray:
    """The demo's five boxes plus MORE_BOXES, truncated to `count`."""
    return np.concatenate([demo_boxes(), MORE_BOXES])[:count].copy()


def demo_plus(*rows) -> np.ndarray:
    """The demo's five boxes with `rows` appended."""
    return np.concatenate([demo_boxes(), np.array(rows, dtype=np.float32).reshape(-1, 4)])


def random_boxes(count: int, W: float, H: float, seed: int, hmax: float, clear: float,
                 planted: Optional[tuple] = None, root: tuple = ROOT_STATE) -> np.ndarray:
    """`count` seeded boxes with centres over [-1, W+1] x [-1, H+1] (some partly or wholly
    outside the workspace) and a clear disc round the root; `planted` replaces row 0."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-1.0, W + 1.0, count), rng.uniform(-1.0, H + 1.0, count)], axis=1).astype(np.float32)
    h = rng.uniform(0.02, hmax, size=(count, 2)).astype(np.float32)
    near = np.hypot(c[:, 0] - root[0], c[:, 1] - root[1]) <= clear
    c[near] += np.float32(2.0 * clear + 2.0 * hmax)   # moved off the disc, not dropped: the count stays
    obs = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    if planted is not None:
        obs[0] = np.array(planted, dtype=np.float32)
    return obs


@dataclass(frozen=True)
class Scenario:
    name: str
    family: str
    targets: str                         # the shortcut this scenario is aimed at
    kw: dict                             # planner kwargs over DEMO + BASE
    boxes: Callable[[], np.ndarray]
    initial: tuple = ROOT_STATE          # (x, y, theta, v)
    goal: tuple = GOAL
    seed: int = BASE_SEED
    env: dict = field(default_factory=dict)   # SBMP_STEP / SBMP_EXPAND_VARIANT
    local_group: int = 0
    obstacle_form: str = "registers"
    cover: tuple = ("spread",)           # coverage conditions (tests/test_scenarios_oracle.py)
    added_rows: tuple = ()               # family F: rows of boxes() that are the added boxes

    @property
    def step_form(self) -> str:
        return "two-launch" if self.env.get("SBMP_STEP") == "0" else "k_step"

    def config(self):
        """(cfg, extra): the KGMT positional configuration and its keyword extras."""
        full = dict(DEMO)
        full.update(BASE)
        full.update(self.kw)
        extra = {k: full.pop(k) for k in EXTRA_KEYS if k in full}
        return full, extra

    def initial7(self):
        return tuple(self.initial) + (0.0, 0.0, 0.0)

    def goal7(self):
        return tuple(self.goal) + (0.0,) * 5

    def obstacles(self) -> np.ndarray:
        return np.ascontiguousarray(self.boxes(), dtype=np.float32).reshape(-1, 4)


def make_oracle(sc: Scenario, obstacles: Optional[np.ndarray] = None, threads: int = 8, plan: bool = True):
    """Run the CPU oracle on a scenario (optionally with another box list); returns it.
    plan=False stops after begin(): the caller steps it."""
    from oracle.pyoracle import Oracle, PlannerConfig
    cfg, extra = sc.config()
    pc = PlannerConfig(**cfg, samplesPerIteration=extra.get("samplesPerIteration", 0),
                       agent=1 if extra.get("agent", "car") == "point" else 0,
                       fixGNewClear=int(extra.get("fixGNewClear", 0)),
                       batchRule=1 if extra.get("batchRule", "reference") == "fill" else 0)
    o = Oracle(pc, threads=threads)
    o.begin(sc.initial7(), sc.goal7(), sc.obstacles() if obstacles is None else obstacles, sc.seed)
    while plan and o.step():
        pass
    return o


def _build() -> list:
    S = []

    def add(name, family, targets, kw=None, boxes=demo_boxes, **rest):
        S.append(Scenario(name=name, family=family, targets=targets, kw=dict(kw or {}), boxes=boxes, **rest))

    sched = ("spread", "schedule")

    # ---- base: the schedule with one or two parents per wave, and car_cull below k = 64
    add("base", "base", "car_schedule valid (64 <= k < 256, two parents per wave) and car_cull (k < 64)", cover=sched)

    # ---- A. non-square workspace: every place that takes W and H separately
    #      (wh in car_euler_fast, far in wave_cull, dw in car_schedule, the oob tests of
    #      car_euler / point_euler, gridInvW / gridInvH), and bins_k's R1Size = W / N on both axes
    for W, H, goal in ((30.0, 12.0, (27.0, 10.0)), (12.0, 30.0, (10.0, 27.0))):
        tag = f"{W:g}x{H:g}"
        reach = ("spread", ("tree_x_beyond", H)) if W > H else ("spread", ("uncounted_y_beyond", W))
        for agent in ("car", "point"):
            # the point moves at most 1.05 per iteration: on (30, 12) it starts where x > H already
            # on (12, 30) the demo's wall (0, 6)-(18, 8) spans the whole width: the root stands above it
            root = (14.0, 5.0, 0.0, 0.0) if (agent == "point" and W > H) else ROOT_STATE if W > H else (5.0, 10.0, 0.0, 0.0)
            r600 = lambda W=W, H=H, root=root: random_boxes(600, W, H, 7, 0.3, 0.8, root=root)
            r3000 = lambda W=W, H=H, root=root: random_boxes(3000, W, H, 11, 0.08, 0.5, root=root)
            kw = dict(width=W, height=H, agent=agent)
            t = "W != H in " + ("car_euler_fast wh / car_schedule dw / wave_cull far" if agent == "car"
                                else "point_euler oob / wave_cull far")
            common = dict(initial=root, goal=goal, cover=reach)
            add(f"A-{tag}-{agent}-registers", "A", t + ", register boxes", kw, **common)
            add(f"A-{tag}-{agent}-lds", "A", "W != H in the oob test of the LDS list form", kw, r600,
                obstacle_form="lds", **common)
            add(f"A-{tag}-{agent}-grid", "A", "gridInvW != gridInvH in the forced grid (grid_run)", kw, r600,
                env={"SBMP_EXPAND_VARIANT": "4"}, obstacle_form="grid", **common)
            add(f"A-{tag}-{agent}-grid-auto", "A", "gridInvW != gridInvH, grid chosen by the box count", kw, r3000,
                obstacle_form="grid", **common)
            add(f"A-{tag}-{agent}-global", "A", "W != H in the oob test of the global all-boxes loop", kw, r3000,
                env={"SBMP_EXPAND_VARIANT": "5"}, obstacle_form="global", **common)
    # R1Size = 17.3 / 16 is not representable: bins_k through div_by or the IEEE branch,
    # whichever the host's reciprocal check picks
    for agent in ("car", "point"):
        kw = dict(width=17.3, height=20.0, agent=agent)
        add(f"A-17.3x20-{agent}-registers", "A", "bins_k with a non-representable R1Size (div_by or IEEE)", kw)
        add(f"A-17.3x20-{agent}-grid", "A", "bins_k with a non-representable R1Size, forced grid", kw,
            lambda: random_boxes(600, 17.3, 20.0, 7, 0.3, 0.8), env={"SBMP_EXPAND_VARIANT": "4"}, obstacle_form="grid")

    # ---- B. root heading at the reduction limits (registers, demo boxes, L = 1)
    add("B-theta+105610", "B", "children cross Cody-Waite's 105615 upwards and back inside the Euler loop (PH form)",
        initial=(5.0, 5.0, 105610.0, 1.0), cover=("spread", ("cross_both", CW_LIMIT)))
    add("B-theta-105612", "B", "children cross -105615 both ways inside the Euler loop (PH form)",
        initial=(5.0, 5.0, -105612.0, 1.0), cover=("spread", ("cross_both", CW_LIMIT)))
    add("B-theta+99995", "B", "lanes on both sides of car_theta_bounded's 100000 in one wave",
        initial=(5.0, 5.0, 99995.0, 1.0), cover=("spread", ("cross_up", BOUNDED_LIMIT)))
    add("B-theta+3e5", "B", "every lane takes Payne-Hanek (car_euler_fast<.., true>)",
        initial=(5.0, 5.0, 3e5, 0.0))
    add("B-theta+1e9", "B", "Payne-Hanek at a heading whose float spacing is 64",
        initial=(5.0, 5.0, 1e9, 0.0))

    # ---- C. power-of-two wheelbase != 1: car_euler_fast<.., false, false>, vl = v * invL
    add("C-L2", "C", "car_euler_fast<OBS, false, false>: vl = v * 0.5", dict(agentLength=2.0), seed=1, cover=sched)
    add("C-L0.5", "C", "car_euler_fast<OBS, false, false>: vl = v * 2", dict(agentLength=0.5), cover=sched)
    add("C-L2^-10", "C", "the PH form with invL != 1: theta passes both limits on its own",
        dict(agentLength=2.0 ** -10), seed=1, cover=sched + (("cross_both", CW_LIMIT),))
    add("C-L2-theta+105610", "C", "invL != 1 in car_theta_bounded's bound at the Cody-Waite limit",
        dict(agentLength=2.0), initial=(5.0, 5.0, 105610.0, 1.0), seed=3,
        cover=sched + (("cross_both", CW_LIMIT),))
    add("C-L2-30x12", "C", "invL != 1 together with W != H", dict(agentLength=2.0, width=30.0, height=12.0),
        goal=(27.0, 10.0), cover=sched + (("tree_x_beyond", 12.0),))

    # ---- D. moving root: the schedule's v term, and the break's "new (x, y), old (theta, v)"
    add("D-v+40", "D", "car_schedule's t v term; most children leave the workspace",
        initial=(5.0, 5.0, 0.7, 40.0))
    add("D-v-25", "D", "car_schedule's |v| with a negative speed", initial=(5.0, 5.0, 2.0, -25.0))
    add("D-corner", "D", "dw in car_schedule / far in wave_cull 0.05 from two walls",
        initial=(0.05, 19.95, 0.3, 2.0))

    # ---- E. (NOBS + 1) numDisc on either side of car_schedule's 64
    #      (with one box or none the root stands nearer the walls, or under 5% of the children are invalid)
    near_wall = {1: ((1.5, 5.0, 0.0, 0.0), 22), 0: ((1.0, 1.0, 0.0, 0.0), 2)}
    for boxes, disc in ((7, 8), (3, 16), (1, 32), (0, 64), (4, 13), (0, 65)):
        prod = (boxes + 1) * disc
        root, seed = near_wall.get(boxes, (ROOT_STATE, BASE_SEED))
        add(f"E-{boxes}boxes-{disc}steps", "E",
            f"(NOBS + 1) numDisc = {prod}: " + ("the bounds bits reach bit 63" if prod == 64 else "no schedule"),
            dict(numDisc=disc), lambda boxes=boxes: demo_prefix(boxes), initial=root, seed=seed, cover=sched)

    # ---- F. degenerate boxes (registers): the obsNaN fallback, the predicates at equality
    #      (F-touching-root / -next is one comparison, o.z <= minx, at the root, in the register fast loop;
    #      the full set -- all four comparisons and both movable walls, at equality and one ulp either
    #      side, in every obstacle form -- is family H, tests/edge_scenarios.py, which derives its boxes
    #      from an oracle pass and so lives outside this oracle-free module)
    nan = float("nan")
    inf = float("inf")
    nan_low = (nan, 4.0, 7.0, 4.5)
    nan_high = (3.0, 5.5, nan, 6.0)
    changes = ("spread", "box_changes")
    for L, ltag in ((1.0, ""), (2.0, "-L2"), (1.3, "-L1.3")):
        # L = 2 and 1.3: car_euler's two v / L branches under obsNaN (car_fast_ok false)
        t = "obsNaN: car_fast_ok false, wave_cull keeps every box" + ("" if L == 1.0 else f", car_euler with L = {L:g}")
        add(f"F-nan-low{ltag}", "F", t, dict(agentLength=L), lambda: demo_plus(nan_low), cover=changes, added_rows=(5,))
        add(f"F-nan-high{ltag}", "F", t, dict(agentLength=L), lambda: demo_plus(nan_high), cover=changes,
            added_rows=(5,))
    # every coordinate NaN: the reference's predicate meets it everywhere (the run stalls,
    # D7), the separation metric of the fast loop would never meet it
    add("F-nan-all", "F", "obsNaN with a box the separation metric cannot see at all",
        boxes=lambda: demo_plus((nan, nan, nan, nan)), cover=("stall", "box_changes"), added_rows=(5,))
    add("F-inf-wall", "F", "infinite box coordinates in wave_cull / car_schedule / box_sep",
        boxes=lambda: demo_plus((12.0, -inf, 13.0, inf)), cover=changes, added_rows=(5,))
    add("F-inverted", "F", "a box inverted by 0.05 beside the root: the metric against the predicate",
        boxes=lambda: demo_plus((5.55, 4.0, 5.5, 6.0)), cover=changes, added_rows=(5,))
    add("F-zero-area", "F", "two zero-area boxes through the root's cell",
        boxes=lambda: demo_plus((6.0, 1.0, 6.0, 9.0), (1.0, 5.5, 9.0, 5.5)), cover=changes, added_rows=(5, 6))
    add("F-touching-root", "F", "o.z <= minx at equality: the root on the box's edge",
        boxes=lambda: demo_plus((2.0, 4.5, 4.0, 5.5)), initial=(4.0, 5.0, 0.0, 0.0), cover=changes, added_rows=(5,))
    add("F-touching-root-next", "F", "o.z <= minx one ulp past equality",
        boxes=lambda: demo_plus((2.0, 4.5, 4.0, 5.5)),
        initial=(float(np.nextafter(np.float32(4.0), np.float32(5.0))), 5.0, 0.0, 0.0), cover=changes, added_rows=(5,))
    add("F-covering", "F", "a box over the whole workspace: every child invalid, the run stalls (D7)",
        boxes=lambda: demo_plus((-1.0, -1.0, 21.0, 21.0)), cover=("stall", "box_changes"), added_rows=(5,))
    add("F-outside", "F", "a box wholly outside the workspace changes nothing",
        boxes=lambda: demo_plus((21.0, 22.0, 24.0, 23.0)), cover=("spread", "box_neutral"), added_rows=(5,))
    nan_planted = (nan, 3.0, 9.0, 3.4)
    add("F-nan-30x12-lds", "F", "a NaN box in the LDS list (the compare form handles it)",
        dict(width=30.0, height=12.0), lambda: random_boxes(600, 30.0, 12.0, 7, 0.3, 0.8, nan_planted),
        goal=(27.0, 10.0), obstacle_form="lds", cover=changes, added_rows=(0,))
    add("F-nan-30x12-grid", "F", "obsNaN in the grid: the batched reference form, not the unmasked query",
        dict(width=30.0, height=12.0), lambda: random_boxes(600, 30.0, 12.0, 7, 0.3, 0.8, nan_planted),
        goal=(27.0, 10.0), env={"SBMP_EXPAND_VARIANT": "4"}, obstacle_form="grid", cover=changes, added_rows=(0,))

    # ---- G. forms: the two-launch form's call into the same fast loop (k_expand, SBMP_STEP=0), shard groups
    by_name = {s.name: s for s in S}

    def again(src, suffix, targets, **changes_):
        s = by_name[src]
        fields = dict(name=f"G-{src}-{suffix}", family="G", targets=targets, kw=dict(s.kw), boxes=s.boxes,
                      initial=s.initial, goal=s.goal, seed=s.seed, env=dict(s.env), local_group=s.local_group,
                      obstacle_form=s.obstacle_form, cover=s.cover, added_rows=s.added_rows)
        fields.update(changes_)
        S.append(Scenario(**fields))

    for src in ("B-theta+105610", "B-theta+99995", "C-L2", "C-L2^-10", "E-7boxes-8steps", "E-4boxes-13steps",
                "F-nan-low-L2"):
        again(src, "two-launch", "k_expand's dispatch: " + by_name[src].targets,
              env=dict(by_name[src].env, SBMP_STEP="0"))
    for src in ("A-30x12-car-registers", "C-L2-theta+105610", "D-v+40"):
        again(src, "group2", "sharded k_step, 2 ranks: " + by_name[src].targets, local_group=2)
    again("A-12x30-car-grid", "group8", "sharded k_step, 8 ranks, LDS grid table: " + by_name["A-12x30-car-grid"].targets,
          local_group=8)
    return S


SCENARIOS = _build()
IDS = [s.name for s in SCENARIOS]
assert len(set(IDS)) == len(IDS)

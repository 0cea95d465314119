"""Family H, "verdict edges": the collision and workspace predicates at equality and one
ulp either side, in every form that restates them.

The reference's predicate (collisionCheck.cu:6-14) is four comparisons,

    free  iff  maxx <= o.x  or  o.z <= minx  or  maxy <= o.y  or  o.w <= miny,

and its workspace test (statePropagator.cu:42-45) x <= 0 or x >= W or y <= 0 or y >= H.
The kernels restate both several times over (box_sep's separation metric with
aliveF = min(in4, sep + 2^-149), box_overlap under motion_valid_culled, the LDS loops,
grid_run_sep behind the grid index, the batched reference form under obsNaN, the
early-exit global loop, point_euler, the public headers behind sbmp_expand_batch).
Random and demo boxes essentially never put a step box within an ulp of a box edge, so
`<` for `<=`, a `sep >= 0` trick that loses the zero, or a grid cell range one ulp short
pass every other test.  Here the edge is put on a child's own float.

Construction.  Iteration 1 expands the root alone, and a child's controls depend only on
seed and slot.  So a pass without planted boxes (pass 0) gives every child's end point bit
for bit, and a second run can put a box edge or a wall on that float:

  box    four slabs, one per comparison, each beyond one extreme valid child (largest x,
         smallest x, largest y, smallest y) with its near edge on that child's coordinate
         (`at`), one ulp towards the child (`in`: the four extremes collide in their last
         step, nobody else changes) or one ulp away (`out`).  0 / 4 / 0 children flip.  A
         collision keeps the step's new state, so every child that was valid in pass 0 is
         stored bit for bit as in pass 0 in all three variants (with one Euler step the
         whole child array is: the workspace test comes before the boxes; with more steps
         a child that left the workspace in pass 0 may stop on a slab before it does).
  wall   width on the +x-most child's x and height on the +y-most child's y: `at` tests
         nx >= W and ny >= H at equality (both out), `in` is one ulp up (both inside),
         `out` one ulp down (both out).  The four slabs stand 0.5 beyond the extremes, so
         the form keeps its box count.  R1Size moves with width: the oracle decides what
         else changes.  The walls at 0 cannot be moved (x <= 0 is a constant of the
         reference): D-corner of tests/scenarios.py stays their nearest test.
  mid    one slab; a probe pass puts it at half the +x extreme's reach, and of the children
         that stop on it before their last step the one with the smallest stopping x gives
         the edge.  At `at` and `out` that child passes the step it died in, at `in` it dies
         there: the schedule's bit (i, k) for i < D - 1, and the grid walk inside a child.

The slab that faces a fast root's heading (the roots of rows 1, 2 and 4 head east, north,
west and south in turn, so each comparison gets its turn) lies at the edge of the reach
bound the conservative culls test the child under: T |v0| + |a| T^2 / 2 for car_cull / wave_cull
(own T and a), t |v0| + 2.5 t^2 at t = D * 1.06 / D for car_schedule's last step, T |vx|
and T |vy| per axis for the point.  The ratio (L-inf displacement of the chosen child over
that radius, from the stored controls) is a property of the oracle's run.  REACH holds the
measured figure of every box case, rounded down to two decimals, and
tests/test_edge_scenarios_oracle.py asserts each as a floor.  One root cannot put all four
comparisons at the reach edge, so only the case that faces the heading is near 1; rows 1, 2
and 4 turn the root instead, rows 3, 11 and 12 have the east heading alone.  Measured, in
the order +x, -x, +y, -y for a root heading east (the other headings are this row turned):

    form                           radius      measured
    H1-fast-sched-{E,N,W,S}        schedule    0.960 0.257 0.640 0.636
    H2-fast-cull-{E,N,W,S}         car_cull    0.978 0.603 0.683 0.663
    H3-fast-L2                     schedule    0.964 0.270 0.624 0.642
    H4-euler-L1.3-{E,N,W,S}        wave_cull   0.979 0.323 0.697 0.646
    H5-point                       per axis    1.000 1.000 1.000 1.000 (the cull's margin is r * 1.0001 + 1e-3)
    H11-two-launch, H12-group2     schedule    as H1-fast-sched-E
    H13-one-step-fast-{NE,SW}      schedule    0.402 (both cases: one child; a root at |v| = 3 heading 0.7)
    H13-one-step-euler-L1.3-..     wave_cull   0.753
    H13-one-step-point             per axis    1.000 1.000 1.000 1.000

The LDS, grid and global forms have no cull.  Their fillers (seeded boxes all over the
workspace) are moved off the chosen children's paths, so the extremes stay the far-reaching
children of the run without boxes while the fillers stop most of the others.

Flip counts measured on the oracle, and the same on the GPU (tests/test_gpu_edge_scenarios.py
on an MI355X): box 0 / 4 / 0 in every multi-step form and for the point; 0 / 1 / 0 for a
car's single step, whose children lie on one ray, so that one child is the extreme of both
axes ahead of the root (the root moving forwards takes +x and +y, in reverse -x and -y);
wall: the chosen pair (one child for a car's single step) out / inside / out; mid: the one
chosen child, and no other, differs between `at` and `in`.

Plain numpy plus the CPU oracle (at call time, not at import); no GPU.  (The header tests of
tests/test_edge_scenarios_oracle.py also call the built library, as tests/test_batch.py does.)
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from scenarios import BASE_SEED, Scenario, make_oracle, random_boxes

SLOTS = 16384
VARIANTS = ("at", "in", "out")
CASES = ("+x", "-x", "+y", "-y")          # maxx <= o.x, o.z <= minx, maxy <= o.y, o.w <= miny
PI = float(np.pi)

# a fast root per heading, 15.5 (the schedule's reach at v = 12) inside the far wall
ROOTS = {"E": (4.0, 10.0, 0.05, 12.0), "N": (10.0, 4.0, PI / 2 + 0.05, 12.0),
         "W": (16.0, 10.0, PI + 0.05, 12.0), "S": (10.0, 16.0, -PI / 2 + 0.05, 12.0)}
ONE_STEP_ROOT = (5.0, 5.0, 0.7, 3.0)
ONE_STEP_BACK = (5.0, 5.0, 0.7, -3.0)


@dataclass(frozen=True, eq=False)
class Form:
    name: str
    row: int                              # row of the issue's form table
    kw: dict
    root: tuple = ROOTS["E"]
    heading: str = "E"
    env: dict = field(default_factory=dict)
    local_group: int = 0
    obstacle_form: str = "registers"
    fillers: int = 0                      # boxes in all, the planted four included (0: only those)
    nan_filler: bool = False
    radius: str = ""                      # "schedule", "cull", "point" or "" (no cull in this form)
    mid: bool = False
    seed: int = BASE_SEED
    cases: tuple = CASES
    groups: tuple = ("box", "wall")

    @property
    def step_form(self) -> str:
        return "two-launch" if self.env.get("SBMP_STEP") == "0" else "k_step"

    @property
    def one_step(self) -> bool:
        return self.kw.get("numDisc", 10) == 1

    @property
    def flips(self) -> int:
        """Children the box case flips at `in`: one per comparison, but one in all for a car's single step."""
        return 1 if self.one_step and self.kw.get("agent") != "point" else len(self.cases)

    def __str__(self):
        return self.name


def _forms() -> list:
    F = []

    def add(name, row, kw=None, **rest):
        F.append(Form(name=name, row=row, kw=dict(kw or {}), **rest))

    for h, root in ROOTS.items():
        add(f"H1-fast-sched-{h}", 1, dict(numDisc=10), root=root, heading=h, radius="schedule",
            mid=(h == "E"))
        add(f"H2-fast-cull-{h}", 2, dict(numDisc=13), root=root, heading=h, radius="cull")
        add(f"H4-euler-L1.3-{h}", 4, dict(agentLength=1.3), root=root, heading=h, radius="cull")
    # (L = 2 turns half as fast: at heading 0.05 a valid child swings past the -y extreme and back)
    add("H3-fast-L2", 3, dict(agentLength=2.0), root=(4.0, 10.0, 0.0, 12.0), radius="schedule")
    # (seed 5 gives the point one child that is both its +x and its +y extreme)
    add("H5-point", 5, dict(agent="point"), radius="point", seed=1)
    add("H6-lds", 6, fillers=600, obstacle_form="lds")
    add("H6-lds4", 6, fillers=600, obstacle_form="lds", env={"SBMP_EXPAND_VARIANT": "2"})
    add("H7-grid-lds-table", 7, fillers=600, obstacle_form="grid", env={"SBMP_EXPAND_VARIANT": "4"}, mid=True)
    add("H8-grid-global-table", 8, fillers=600, obstacle_form="grid",
        env={"SBMP_EXPAND_VARIANT": "4", "SBMP_STEP": "0"}, mid=True)
    add("H9-global", 9, fillers=3000, obstacle_form="global", env={"SBMP_EXPAND_VARIANT": "5"})
    add("H10-grid-nan", 10, fillers=600, obstacle_form="grid", env={"SBMP_EXPAND_VARIANT": "4"}, nan_filler=True)
    add("H11-two-launch", 11, radius="schedule", env={"SBMP_STEP": "0"})
    add("H12-group2", 12, radius="schedule", local_group=2)
    add("H12-group2-grid", 12, fillers=600, obstacle_form="grid", env={"SBMP_EXPAND_VARIANT": "4"}, local_group=2)
    # One Euler step moves a car child along the root's heading by v T: the children lie on a ray, the
    # longest is the extreme of both axes ahead of the root, and nothing lies behind it.  So a root
    # moving up and right takes the +x and +y comparisons and the walls, the same root in reverse the
    # -x and -y comparisons; the point's children spread to all four sides.
    one = dict(numDisc=1)
    for tag, root, cases, groups in (("NE", ONE_STEP_ROOT, ("+x", "+y"), ("box", "wall")),
                                     ("SW", ONE_STEP_BACK, ("-x", "-y"), ("box",))):
        common = dict(root=root, heading=tag, cases=cases, groups=groups)
        add(f"H13-one-step-fast-{tag}", 13, one, radius="schedule", **common)
        add(f"H13-one-step-euler-L1.3-{tag}", 13, dict(one, agentLength=1.3), radius="cull", **common)
        add(f"H13-one-step-lds-{tag}", 13, one, fillers=600, obstacle_form="lds", **common)
        add(f"H13-one-step-grid-{tag}", 13, one, fillers=600, obstacle_form="grid",
            env={"SBMP_EXPAND_VARIANT": "4"}, **common)
        add(f"H13-one-step-global-{tag}", 13, one, fillers=3000, obstacle_form="global",
            env={"SBMP_EXPAND_VARIANT": "5"}, **common)
    add("H13-one-step-point", 13, dict(one, agent="point"), root=ONE_STEP_ROOT, radius="point", seed=1)
    return F


FORMS = _forms()

# Floors of the reach ratio per box case, in the order of the form's cases (+x, -x, +y, -y): the
# figure measured on the oracle (in the comment), rounded down to two decimals.
REACH = {
    "H1-fast-sched-E": (0.95, 0.25, 0.63, 0.63),              # 0.9600 0.2572 0.6398 0.6358
    "H2-fast-cull-E": (0.97, 0.60, 0.68, 0.66),               # 0.9783 0.6032 0.6825 0.6628
    "H4-euler-L1.3-E": (0.97, 0.32, 0.69, 0.64),              # 0.9785 0.3234 0.6970 0.6461
    "H1-fast-sched-N": (0.63, 0.63, 0.95, 0.25),              # 0.6358 0.6398 0.9600 0.2572
    "H2-fast-cull-N": (0.66, 0.68, 0.97, 0.60),               # 0.6628 0.6825 0.9783 0.6032
    "H4-euler-L1.3-N": (0.64, 0.69, 0.97, 0.32),              # 0.6461 0.6970 0.9785 0.3234
    "H1-fast-sched-W": (0.25, 0.95, 0.63, 0.63),              # 0.2572 0.9600 0.6358 0.6398
    "H2-fast-cull-W": (0.60, 0.97, 0.66, 0.68),               # 0.6032 0.9783 0.6628 0.6825
    "H4-euler-L1.3-W": (0.32, 0.97, 0.64, 0.69),              # 0.3234 0.9785 0.6461 0.6970
    "H1-fast-sched-S": (0.63, 0.63, 0.25, 0.95),              # 0.6398 0.6358 0.2572 0.9600
    "H2-fast-cull-S": (0.68, 0.66, 0.60, 0.97),               # 0.6825 0.6628 0.6032 0.9783
    "H4-euler-L1.3-S": (0.69, 0.64, 0.32, 0.97),              # 0.6970 0.6461 0.3234 0.9785
    "H3-fast-L2": (0.96, 0.27, 0.62, 0.64),                   # 0.9641 0.2701 0.6235 0.6416
    "H5-point": (1.00, 1.00, 1.00, 1.00),                     # 1.0000 each (just above: the cull's margin covers it)
    "H11-two-launch": (0.95, 0.25, 0.63, 0.63),               # as H1-fast-sched-E
    "H12-group2": (0.95, 0.25, 0.63, 0.63),                   # as H1-fast-sched-E
    "H13-one-step-fast-NE": (0.40, 0.40),                     # 0.4023 (one child carries both cases)
    "H13-one-step-euler-L1.3-NE": (0.75, 0.75),               # 0.7532
    "H13-one-step-fast-SW": (0.40, 0.40),                     # 0.4023
    "H13-one-step-euler-L1.3-SW": (0.75, 0.75),               # 0.7532
    "H13-one-step-point": (1.00, 0.99, 1.00, 0.99),           # 1.0000 each, two of them just below
}
FORM_IDS = [f.name for f in FORMS]
assert len(set(FORM_IDS)) == len(FORM_IDS)
MID_FORMS = [f for f in FORMS if f.mid]
W0 = H0 = 20.0                            # pass 0's workspace (the demo's)
FAR = 40.0                                # a filler moved off a chosen child's path goes this far out


def up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def down(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def scenario(form: Form, boxes: np.ndarray, width: float = W0, height: float = H0) -> Scenario:
    kw = dict(form.kw, numIterations=3, width=float(width), height=float(height))
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    return Scenario(name=form.name, family="H", targets="verdict edges", kw=kw, boxes=lambda: boxes,
                    initial=form.root, seed=form.seed, env=dict(form.env), local_group=form.local_group,
                    obstacle_form=form.obstacle_form)


def planner_config(sc: Scenario):
    from oracle.pyoracle import PlannerConfig
    cfg, extra = sc.config()
    return PlannerConfig(**cfg, samplesPerIteration=extra["samplesPerIteration"],
                         agent=1 if extra.get("agent", "car") == "point" else 0, fixGNewClear=1, batchRule=1)


def iteration1(sc: Scenario):
    """(children (SLOTS, 7), valid (SLOTS,)) of the oracle's first iteration: the root's children as the
    planner stores them, and each one's verdict from a replay of its stored controls."""
    from oracle.pyoracle import replay
    o = make_oracle(sc, plan=False)
    assert o.step()
    u, up_ = o.unexplored()
    u = u[:SLOTS].copy()
    assert (up_[:SLOTS] == 0).all()
    parents = np.tile(np.asarray(sc.initial, dtype=np.float32), (SLOTS, 1))
    states, valid = replay(planner_config(sc), sc.obstacles(), parents, u[:, 4:7])
    assert np.array_equal(states.view(np.uint32), u[:, :4].view(np.uint32)), "the replay is the planner's child"
    reg = o.regions()
    # the planner counted what the replay says (cells inside the R1 grid only, the root's seed apart)
    assert int(reg["R1Valid"].sum()) - 1 <= int(valid.sum()) and int(reg["R1Invalid"].sum()) <= int((~valid).sum())
    return u, valid


def _extremes(form: Form, u, valid):
    idx = np.nonzero(valid)[0]
    assert len(idx) > 100
    ext, coord = {}, {}
    for case in form.cases:
        col = u[idx, 0 if case[1] == "x" else 1]
        best = col.max() if case[0] == "+" else col.min()
        hit = idx[col == best]
        assert len(hit) == 1, f"{form.name} {case}: {len(hit)} children share the extreme"
        ext[case], coord[case] = int(hit[0]), np.float32(best)
    return ext, coord


@functools.lru_cache(maxsize=None)
def _bare(form: Form):
    sc = scenario(form, np.zeros((0, 4), dtype=np.float32))
    u, valid = iteration1(sc)
    return sc, u, _extremes(form, u, valid)[0]


def bare_extremes(form: Form) -> dict:
    """case -> slot of the extreme valid child of the run without any box."""
    return dict(_bare(form)[2])


@functools.lru_cache(maxsize=None)
def filler_rows(form: Form) -> np.ndarray:
    """The form's boxes past the planted ones (rows 4 ..), none for a register form: seeded boxes all
    over the workspace, those on the path of a chosen child (the extremes of a run without any box)
    moved out of the way, so that the fillers thin out the children and leave the extremes the
    far-reaching ones."""
    from oracle.pyoracle import replay
    if not form.fillers:
        return np.zeros((0, 4), dtype=np.float32)
    hmax, clear, seed = (0.3, 0.8, 7) if form.fillers <= 600 else (0.08, 0.5, 11)
    rows = random_boxes(form.fillers, W0, H0, seed, hmax, clear, root=form.root)[4:]
    bare, u, ext = _bare(form)
    chosen = sorted(set(ext.values()))
    pc = planner_config(bare)
    parents = np.tile(np.asarray(form.root, dtype=np.float32), (len(chosen), 1))

    def clear_of(boxes):
        return replay(pc, boxes, parents, u[chosen, 4:7], threads=1)[1].all()

    for r in range(len(rows)):
        if not clear_of(rows[r:r + 1]):
            rows[r, [0, 2]] += np.float32(FAR)
    if form.nan_filler:
        # (NaN, y0, x1, y1) meets every step box with minx < x1 in its y range: one that ends behind
        # the root shadows a strip there
        for r in np.nonzero((rows[:, 2] > 0.5) & (rows[:, 2] < form.root[0] - 1.0))[0]:
            trial = rows[r:r + 1].copy()
            trial[0, 0] = np.nan
            if clear_of(trial):
                rows[r] = trial[0]
                break
        assert np.isnan(rows).sum() == 1
    assert clear_of(rows)
    rows.setflags(write=False)
    return rows


@dataclass(frozen=True, eq=False)
class Pass0:
    children: np.ndarray
    valid: np.ndarray
    extremes: dict        # case -> slot of the extreme valid child
    coord: dict           # case -> that child's coordinate (np.float32)

    @property
    def chosen(self) -> list:
        return sorted(set(self.extremes.values()))


@functools.lru_cache(maxsize=None)
def pass0(form: Form) -> Pass0:
    u, valid = iteration1(scenario(form, filler_rows(form)))
    ext, coord = _extremes(form, u, valid)
    # one child per comparison, but for a car's single step (see _forms)
    assert len(set(ext.values())) == form.flips
    return Pass0(u, valid, ext, coord)


def slabs(form: Form, coord: dict, variant: str, shift: float = 0.0) -> np.ndarray:
    """The four planted boxes with their near edges on `coord` (shift > 0: that far beyond).  A side
    the form has no case for gets its slab 0.5 behind the root, where no child goes."""
    lo, hi = {"at": (lambda v: v, lambda v: v), "in": (down, up), "out": (up, down)}[variant]
    s, half = np.float32(shift), np.float32(0.5)
    x0, y0 = np.float32(form.root[0]), np.float32(form.root[1])
    px = lo(coord["+x"] + s) if "+x" in coord else x0 + half      # slab beyond the +x extreme: its low edge o.x
    mx = hi(coord["-x"] - s) if "-x" in coord else x0 - half      # beyond the -x extreme: its high edge o.z
    py = lo(coord["+y"] + s) if "+y" in coord else y0 + half
    my = hi(coord["-y"] - s) if "-y" in coord else y0 - half
    return np.array([[px, -1.0, px + np.float32(1.0), H0 + 1.0],
                     [mx - np.float32(1.0), -1.0, mx, H0 + 1.0],
                     [-1.0, py, W0 + 1.0, py + np.float32(1.0)],
                     [-1.0, my - np.float32(1.0), W0 + 1.0, my]], dtype=np.float32)


def box_case(form: Form, variant: str) -> Scenario:
    return scenario(form, np.concatenate([slabs(form, pass0(form).coord, variant), filler_rows(form)]))


def wall_case(form: Form, variant: str) -> Scenario:
    p0 = pass0(form)
    move = {"at": lambda v: v, "in": up, "out": down}[variant]
    boxes = np.concatenate([slabs(form, p0.coord, "at", shift=0.5), filler_rows(form)])
    return scenario(form, boxes, width=float(move(p0.coord["+x"])), height=float(move(p0.coord["+y"])))


@functools.lru_cache(maxsize=None)
def mid_probe(form: Form):
    """(slot, stopping x) of the child that stops first on a probe slab at half the +x extreme's reach."""
    p0 = pass0(form)
    X = np.float32(0.5 * (form.root[0] + float(p0.coord["+x"])))
    probe = np.array([[X, -1.0, X + np.float32(1.0), H0 + 1.0]], dtype=np.float32)
    u, valid = iteration1(scenario(form, np.concatenate([probe, filler_rows(form)])))
    moved = (u[:, :4].view(np.uint32) != p0.children[:, :4].view(np.uint32)).any(axis=1)
    cand = np.nonzero(p0.valid & ~valid & moved)[0]     # stopped by the probe before the last step
    assert len(cand) > 10
    xs = u[cand, 0].min()
    hit = cand[u[cand, 0] == xs]
    assert len(hit) == 1 and xs > X
    return int(hit[0]), np.float32(xs)


def mid_case(form: Form, variant: str) -> Scenario:
    _, xs = mid_probe(form)
    X = {"at": lambda v: v, "in": down, "out": up}[variant](xs)
    slab = np.array([[X, -1.0, X + np.float32(1.0), H0 + 1.0]], dtype=np.float32)
    return scenario(form, np.concatenate([slab, filler_rows(form)]))


GROUPS = {"box": box_case, "wall": wall_case, "mid": mid_case}
GROUP_PARAMS = [(f, g) for f in FORMS for g in f.groups] + [(f, "mid") for f in MID_FORMS]
GROUP_IDS = [f"{f.name}-{g}" for f, g in GROUP_PARAMS]


def reach_ratio(form: Form, child: np.ndarray) -> float:
    """L-inf displacement of `child` over the radius the form's cull tests it under, from its stored
    controls (kgmt_device.h: car_cull / wave_cull, car_schedule's last step)."""
    x0, y0, _, v0 = (float(v) for v in form.root)
    dx, dy = abs(float(child[0]) - x0), abs(float(child[1]) - y0)
    T = float(child[6])
    if form.radius == "point":
        return max(dx / (T * abs(float(child[4]))), dy / (T * abs(float(child[5]))))
    if form.radius == "cull":
        r = T * abs(v0) + 0.5 * abs(float(child[4])) * T * T
    else:
        t = 1.06
        r = t * abs(v0) + 2.5 * t * t
    return max(dx, dy) / r


# ---------------------------------------------------------------- the reference's predicates in numpy
def step_boxes(root, children):
    """One Euler step: the step box is min / max of the root and the child (statePropagator.cu:52-60)."""
    x0, y0 = np.float32(root[0]), np.float32(root[1])
    x, y = children[:, 0], children[:, 1]
    return np.minimum(x0, x), np.minimum(y0, y), np.maximum(x0, x), np.maximum(y0, y)


def reference_invalid(root, children, boxes, width, height):
    """Invalid children of a one-step expansion by the reference's own comparisons in float32:
    statePropagator.cu:42-45 (workspace) and collisionCheck.cu:6-28 (free iff, on some axis,
    bbMax[d] <= obs[d] or obs[2 + d] <= bbMin[d]; invalid iff some box is not free)."""
    children = np.asarray(children, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    W, H = np.float32(width), np.float32(height)
    x, y = children[:, 0], children[:, 1]
    oob = (x <= 0) | (x >= W) | (y <= 0) | (y >= H)
    minx, miny, maxx, maxy = (a[:, None] for a in step_boxes(root, children))
    ox, oy, oz, ow = (boxes[None, :, k] for k in range(4))
    free = (maxx <= ox) | (oz <= minx) | (maxy <= oy) | (ow <= miny)
    return oob | (~free).any(axis=1)


def in_r1_grid(children, width, N=16):
    """getR1 (KGMT.cu:602-609) != -1: the cells the planner's R1 counters see (both axes by width / N)."""
    size = np.float32(width) / np.float32(N)
    cx = np.trunc(np.asarray(children[:, 0], dtype=np.float32) / size)
    cy = np.trunc(np.asarray(children[:, 1], dtype=np.float32) / size)
    return (cx >= 0) & (cx < N) & (cy >= 0) & (cy < N)

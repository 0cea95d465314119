"""The restatements (the CPU oracle, the public headers on the host, the float32 region model)
against the reference's own text, host-compiled: oracle/_ref/libkgmt_ref.so holds the reference's
propagateAndCheck, isMotionValid, getR1, getR2, getCost and inGoalRegion, compiled unmodified by
`make -C oracle ref` (g++ -ffp-contract=fast standing in for nvcc's -fmad=true, D9's sin / cos /
tan standing in for libdevice's).  Every other parity test of the suite ends at the oracle, which
is this project's reading of those functions; these end at the functions themselves.

  a  propagateAndCheck over batches, against the oracle and the headers
  b  every slot of every iteration of the car scenarios (tests/scenarios.py) and of the verdict
     edges (tests/edge_scenarios.py), replayed through propagateAndCheck
  c  getR1 / getR2 on the region edges (tests/region_scenarios.py) and on the children of (a)
  d  inGoalRegion against the float rule D18, outside a three-ulp band round the radius
  e  getCost, and isMotionValid on NaN, infinite, inverted and zero-area boxes

No GPU.  With the reference tree present nothing here skips; tests/reference_text.py builds the
library.  The point agent has no counterpart in the reference and stays out throughout.
"""
import numpy as np
import pytest

import reference_text as rt
from conftest import bits
from edge_scenarios import FORMS, box_case, pass0, wall_case
from region_scenarios import CASE_IDS, N1, Model, cases, expand_inputs, model_cells, sizes
from scenarios import SCENARIOS, demo_plus, make_oracle
from test_batch import _batch, _obstacle_sets

SHAPES = [(10, 1.0), (7, 1.3), (10, 2.0), (1, 1.0), (64, 0.5)]
K = 4096


@pytest.fixture(scope="module")
def ref(oracle_lib):
    """With the reference tree present (or the library built) every test here runs; only a machine
    with neither has nothing to hold the restatements to."""
    try:
        return rt.lib()
    except FileNotFoundError as e:
        pytest.skip(str(e))


def batch(k, seed, width=20.0, height=20.0):
    """test_batch._batch, its positions scaled to the workspace."""
    parents, states = _batch(k, seed)
    parents[:, 0] *= np.float32(width / 20.0)
    parents[:, 1] *= np.float32(height / 20.0)
    return parents, states


# ---------------------------------------------------------------- a. propagateAndCheck
def check_expand(ref, obs, numDisc, L, width=20.0, height=20.0, k=K):
    from cudasbmp_amd.batch import expand_batch
    parents, states = batch(k, 11 + numDisc, width, height)
    r = ref.ref_expand(parents, states, obs, numDisc, L, width, height)
    o = ref.expand_batch(ref.PlannerConfig(numDisc=numDisc, agentLength=L, width=width, height=height), obs, parents,
                         states)
    h = expand_batch(parents, states, obs, numDisc=numDisc, agentLength=L, width=width, height=height, device=False)
    for name, got in (("oracle", o), ("headers", h)):
        assert np.array_equal(bits(got["children"]), bits(r["children"])), name
        assert np.array_equal(got["valid"].astype(bool), r["valid"]), name
        assert np.array_equal(got["rng"], r["rng"]), name     # no R1Score: three draws each
    share = r["valid"].mean()
    print(f"valid share {share:.3f}")
    assert 0.02 <= share <= 0.98
    return parents, r


@pytest.mark.parametrize("obs_name", ["demo", "none", "c5"])
@pytest.mark.parametrize("numDisc,L", SHAPES)
def test_propagate_and_check(obs_name, numDisc, L, obstacles, ref):
    check_expand(ref, _obstacle_sets(obstacles)[obs_name], numDisc, L)


def test_propagate_and_check_30x12(obstacles, ref):
    check_expand(ref, obstacles, 10, 1.0, width=30.0, height=12.0)


# ---------------------------------------------------------------- b. the replay
# Skipped: the point agent's scenarios (A-*-point-*: the reference has no point agent), and family
# G, whose members are an earlier car scenario with another kernel form or shard group -- settings
# that do not reach the CPU oracle, so their replay would be that scenario's once more.
# Measured on the oracle (12 iterations each; scenario, slots replayed, valid share), every slot identical:
#   base 193,522 0.700   A-30x12-car-registers 178,947 0.636   A-30x12-car-lds 195,171 0.455
#   A-30x12-car-grid 195,171 0.455   A-30x12-car-grid-auto 193,418 0.380   A-30x12-car-global 193,418 0.380
#   A-12x30-car-registers 195,521 0.742   A-12x30-car-lds 162,286 0.520   A-12x30-car-grid 162,286 0.520
#   A-12x30-car-grid-auto 178,409 0.460   A-12x30-car-global 178,409 0.460   A-17.3x20-car-registers 195,354 0.733
#   A-17.3x20-car-grid 194,681 0.478   B-theta+105610 193,062 0.666   B-theta-105612 192,781 0.660
#   B-theta+99995 194,007 0.669   B-theta+3e5 194,071 0.638   B-theta+1e9 193,456 0.513
#   C-L2 195,071 0.636   C-L0.5 193,845 0.730   C-L2^-10 193,581 0.675
#   C-L2-theta+105610 192,673 0.641   C-L2-30x12 195,327 0.640   D-v+40 195,536 0.355
#   D-v-25 191,488 0.452   D-corner 173,216 0.563   E-7boxes-8steps 194,247 0.634
#   E-3boxes-16steps 195,069 0.794   E-1boxes-32steps 194,361 0.814   E-0boxes-64steps 193,523 0.791
#   E-4boxes-13steps 194,851 0.779   E-0boxes-65steps 193,564 0.801   F-nan-low 193,430 0.653
#   F-nan-high 193,852 0.711   F-nan-low-L2 193,857 0.634   F-nan-high-L2 194,140 0.646
#   F-nan-low-L1.3 193,110 0.623   F-nan-high-L1.3 194,165 0.711   F-nan-all 16,384 0.000
#   F-inf-wall 194,873 0.695   F-inverted 193,555 0.676   F-zero-area 193,996 0.617
#   F-touching-root 194,235 0.620   F-touching-root-next 194,235 0.620   F-covering 16,384 0.000
#   F-outside 193,522 0.700   F-nan-30x12-lds 195,090 0.457   F-nan-30x12-grid 195,090 0.457
# 48 scenarios, 8,830,240 slots.  The verdict edges: 59 cases x 3 variants of 3 iterations, 8,455,045 slots,
# valid shares 0.145 .. 0.823 (45,110 to 49,127 slots per run).
CAR_SCENARIOS = [s for s in SCENARIOS if s.family != "G" and rt.is_car(s)]
CAR_FORMS = [f for f in FORMS if f.kw.get("agent") != "point"]
EDGE_PARAMS = [(f, g) for f in CAR_FORMS for g in f.groups]


def check_share(r, stall=False):
    print(f"replayed {r.iterations} iterations, {r.slots} slots, valid share {r.share:.4f}")
    assert r.iterations >= 1 and r.slots > 0
    if not stall:
        assert 0.02 <= r.share <= 0.98


@pytest.mark.parametrize("sc", CAR_SCENARIOS, ids=[s.name for s in CAR_SCENARIOS])
def test_replay_scenarios(sc, ref):
    check_share(rt.replay(make_oracle(sc, plan=False), sc), stall="stall" in sc.cover)


@pytest.mark.parametrize("form,group", EDGE_PARAMS, ids=[f"{f.name}-{g}" for f, g in EDGE_PARAMS])
def test_replay_verdict_edges(form, group, ref):
    """The verdict at equality is the reference's own <= (collisionCheck.cu:10) and >=
    (statePropagator.cu:42): `at` and `out` leave the chosen children free of the slab, `in` stops
    them; a wall `at` or `out` puts the chosen pair outside, `in` keeps it."""
    p0 = pass0(form)
    for variant in ("at", "in", "out"):
        sc = (box_case if group == "box" else wall_case)(form, variant)
        r = rt.replay(make_oracle(sc, plan=False), sc, label=f"{sc.name}-{group}-{variant}")
        check_share(r)
        chosen = p0.chosen if group == "box" else sorted({p0.extremes["+x"], p0.extremes["+y"]})
        want = (variant != "in") if group == "box" else (variant == "in")
        assert (r.first.valid[chosen] == want).all(), f"{variant}: {r.first.valid[chosen]}"


# ---------------------------------------------------------------- c. getR1 / getR2
def defined(xy, R1Size):
    """Where static_cast<int>(x / R1Size) is defined: finite and inside int range.  Outside it the
    reference's text is undefined behaviour and -1 is this project's decision (D3); the reference's
    function is not called there."""
    with np.errstate(all="ignore"):
        q = np.asarray(xy, dtype=np.float32) / np.float32(R1Size)
        return (np.isfinite(q) & (np.abs(q) < 2.0 ** 31)).all(axis=1)


def check_cells(ref, xy, width, n, N=N1, others=()):
    R1Size = np.float32(np.float32(width) / np.float32(N))
    R2Size = np.float32(np.float32(width) / np.float32(n * N))
    if N == N1:
        assert (R1Size, R2Size) == sizes(width, n)
    ok = defined(xy, R1Size)
    assert ok.sum() > 0.9 * len(xy)
    r1, r2 = ref.ref_cells(xy[ok], R1Size, N, R2Size, n)
    h1, h2 = ref.header_cells(xy[ok], R1Size, N, R2Size, n)
    assert np.array_equal(r1, h1) and np.array_equal(r2, h2), "include/sbmp/grid.h"
    if N == N1:
        m1, m2, _ = model_cells(Model(), xy[ok, 0], xy[ok, 1], width, n)
        assert np.array_equal(r1, m1) and np.array_equal(r2, m2), "the float32 model"
    for name, (o1, o2) in others:
        assert np.array_equal(r1, o1[ok]) and np.array_equal(r2, o2[ok]), name
    return r1, r2, ok


# (J-r1-point-*: the point agent has no counterpart in the reference)
CAR_CASE_IDS = [c for c in CASE_IDS if "-point-" not in c]


@pytest.mark.parametrize("name", CAR_CASE_IDS)
def test_cells_on_region_edges(name, ref):
    """The planted inputs of family J (the quotient rounded up onto a cell line, the -1 edge, the
    contracted local coordinate, the R2 gap, both division branches): iteration 1's children of the
    case, as the oracle and the headers expand them, through the reference's getR1 / getR2."""
    from cudasbmp_amd.batch import expand_batch
    case = cases()[name]
    parents, rng = expand_inputs(case)
    assert case.agent == "car"
    obs = np.zeros((0, 4), np.float32)      # the cells do not depend on the boxes
    cfg = ref.PlannerConfig(width=case.width, height=case.height, n=case.n)
    o = ref.expand_batch(cfg, obs, parents, rng)
    h = expand_batch(parents, rng, obs, width=case.width, height=case.height, n=case.n, device=False)
    assert np.array_equal(bits(o["children"]), bits(h["children"]))
    xy = np.ascontiguousarray(o["children"][:, :2])
    r1, r2, ok = check_cells(ref, xy, case.width, case.n,
                             others=(("oracle", (o["r1"], o["r2"])), ("headers via expand", (h["r1"], h["r2"]))))
    assert ok.all()
    if case.target >= 0:    # the planted child is among them, with the cell its kind names
        t, col = case.target, (r1[case.target] % N1, r1[case.target] // N1)[case.axis]
        if case.kind in ("r1-up", "r1-on", "r1-above"):
            assert col == case.c
        elif case.kind == "r1-below":
            assert col == case.c - 1
        elif case.kind in ("minus1-at", "minus1-out"):
            assert r1[t] == -1
        elif case.kind == "minus1-in":
            assert col == 0
        elif case.kind == "gap":
            assert r1[t] >= 0 and r2[t] == -1
        elif case.kind == "fma":
            assert r2[t] >= 0


@pytest.mark.parametrize("W,N,n", [(20.0, 16, 8), (17.3, 16, 8), (20.0, 16, 11), (30.0, 7, 3)])
def test_cells_of_expanded_children(W, N, n, obstacles, ref):
    from cudasbmp_amd.batch import expand_batch
    parents, states = batch(K, 21, W, 20.0)
    cfg = ref.PlannerConfig(width=W, N=N, n=n)
    o = ref.expand_batch(cfg, obstacles, parents, states)
    h = expand_batch(parents, states, obstacles, width=W, N=N, n=n, device=False)
    xy = np.ascontiguousarray(o["children"][:, :2])
    r1, r2, _ = check_cells(ref, xy, W, n, N, others=(("oracle", (o["r1"], o["r2"])), ("headers", (h["r1"], h["r2"]))))
    assert (r1 >= 0).mean() > 0.5 and (r1 < 0).any() and len(np.unique(r1)) > N


# ---------------------------------------------------------------- d. inGoalRegion
GOAL = (2.0, 18.0)
RADII = (0.5, 0.00063, 7.0)


def ring(r, spread, count, seed):
    """Points at distance r (1 + u), u uniform in [-spread, spread], round GOAL."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, count)
    d = np.float32(r) * (1.0 + rng.uniform(-spread, spread, count))
    return np.stack([GOAL[0] + d * np.cos(ang), GOAL[1] + d * np.sin(ang)], axis=1).astype(np.float32)


def goal_verdicts(ref, xy, r):
    a, b = ref.header_goal(xy, GOAL, r)
    return ref.ref_goal(xy, GOAL, r), a, b


@pytest.mark.parametrize("r", RADII)
def test_goal_region_outside_the_band(r, ref):
    """Under g++ pow(float, int) is the double overload, so the reference's text computes the
    distance in double where D18 computes it in float; which overload nvcc picks is not knowable
    here.  More than three float ulps of r away from r the two must agree."""
    xy = ring(r, 0.1, 66667, 7)
    t, a, b = goal_verdicts(ref, xy, r)
    band = rt.goal_band(xy, GOAL, r)
    print(f"r = {r}: {band.sum()} of {len(xy)} in the band, {(t != a).sum()} disagree in all")
    assert band.mean() < 0.01
    assert np.array_equal(a, b), "sbmp::inGoalRegion and goal_inside are one rule"
    assert np.array_equal(t[~band], a[~band])
    assert 0.3 < t.mean() < 0.7


@pytest.mark.parametrize("r", RADII)
def test_goal_region_crowded_on_the_radius(r, ref):
    """Points within about 8 ulps of the radius: inside the band nothing is asserted about the
    verdicts, the disagreeing share is printed (DESIGN.md §3 records the figure measured at a relative
    spread of 1e-6); outside the band the rules agree."""
    xy = ring(r, 8 * 2.0 ** -24, 66667, 9)
    t, a, b = goal_verdicts(ref, xy, r)
    band = rt.goal_band(xy, GOAL, r)
    print(f"r = {r}: {(t != a).sum()} of {len(xy)} verdicts differ; {band.sum()} in the band")
    assert np.array_equal(a, b)
    assert np.array_equal(t[~band], a[~band])


# ---------------------------------------------------------------- e. getCost and isMotionValid
def test_cost(ref):
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-5, 5, size=(512, 7)).astype(np.float32)
    x1 = rng.uniform(-5, 5, size=(512, 7)).astype(np.float32)
    x1[:4, 6] = (np.nan, np.inf, -0.0, 1.05)
    assert np.array_equal(bits(ref.ref_cost(x0, x1)), bits(x1[:, 6]))   # KGMT.cu:631-633: the duration


NAN, INF = float("nan"), float("inf")
# family F's added boxes (tests/scenarios.py), called directly
F_BOXES = {"nan-low": (NAN, 4.0, 7.0, 4.5), "nan-high": (3.0, 5.5, NAN, 6.0), "nan-all": (NAN,) * 4,
           "inf-wall": (12.0, -INF, 13.0, INF), "inverted": (5.55, 4.0, 5.5, 6.0),
           "zero-area-v": (6.0, 1.0, 6.0, 9.0), "zero-area-h": (1.0, 5.5, 9.0, 5.5),
           "covering": (-1.0, -1.0, 21.0, 21.0), "outside": (21.0, 22.0, 24.0, 23.0)}


def numpy_free(lo, hi, box):
    """collisionCheck.cu:10 written out: free iff on some axis bbMax <= obs low or obs high <= bbMin."""
    with np.errstate(invalid="ignore"):
        b = np.asarray(box, dtype=np.float32)
        return (hi[:, 0] <= b[0]) | (b[2] <= lo[:, 0]) | (hi[:, 1] <= b[1]) | (b[3] <= lo[:, 1])


@pytest.mark.parametrize("kind", list(F_BOXES))
def test_motion_valid_on_degenerate_boxes(kind, ref):
    box = np.array([F_BOXES[kind]], dtype=np.float32)
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 20, size=(4096, 2)).astype(np.float32)
    b = (a + rng.uniform(-1.2, 1.2, size=a.shape)).astype(np.float32)
    # step boxes on the box's own coordinates, and degenerate ones (a point, a segment)
    fin = np.where(np.isfinite(box[0]), box[0], np.float32(5.0))
    a[:8] = [(fin[0], fin[1]), (fin[2], fin[3]), (fin[0], 5.0), (fin[2], 5.0), (5.0, fin[1]), (5.0, fin[3]),
             (fin[2], fin[1]), (fin[0], fin[3])]
    b[:4] = a[:4]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    got = ref.ref_motion_valid(lo, hi, box)
    assert np.array_equal(got, numpy_free(lo, hi, box[0]))
    if kind == "nan-all":
        assert not got.any()
    elif kind == "covering":    # the planted step boxes touch its edges from outside: free at equality
        assert not got[8:].any() and got[:2].all()
    elif kind == "outside":
        assert got.all()
    else:
        assert got.any() and not got.all()
    # among other boxes the verdict is the conjunction
    both = ref.ref_motion_valid(lo, hi, demo_plus(F_BOXES[kind]))
    demo = ref.ref_motion_valid(lo, hi, demo_plus())
    assert np.array_equal(both, demo & got)
    assert ref.ref_motion_valid(lo, hi, np.zeros((0, 4), np.float32)).all()


@pytest.mark.parametrize("kind", list(F_BOXES))
def test_one_step_verdict_is_motion_valid(kind, obstacles, ref):
    """The oracle's and the headers' one-step verdict is isMotionValid on the step box of parent and
    child, for the children that stay inside the workspace."""
    from cudasbmp_amd.batch import expand_batch
    obs = demo_plus(F_BOXES[kind])
    parents, states = batch(K, 31)
    o = ref.expand_batch(ref.PlannerConfig(numDisc=1), obs, parents, states)
    h = expand_batch(parents, states, obs, numDisc=1, device=False)
    c = o["children"]
    inside = (c[:, 0] > 0) & (c[:, 0] < 20) & (c[:, 1] > 0) & (c[:, 1] < 20)
    lo, hi = np.minimum(parents[:, :2], c[:, :2]), np.maximum(parents[:, :2], c[:, :2])
    want = inside & ref.ref_motion_valid(lo, hi, obs)
    assert np.array_equal(o["valid"].astype(bool), want) and np.array_equal(h["valid"].astype(bool), want)
    assert not o["valid"][~inside].any()

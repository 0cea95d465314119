"""Adoption on the GPU (tree_adopt.hip; include/sbmp/tree_adopt.h).

  the kernels       sbmp_tree_adopt_tables equals the numpy model and the host twin bit for bit on the
                    whole table (tests/tree_adopt_cases.py); two calls give identical bytes.  Its cases
                    past one sweep of the grid (524,288 rows at most; fewer resident workgroups only
                    start the later rounds sooner) reach the later rounds of k_adopt_scan and k_adopt_seed
  the planner       adopt() then regions(), tree(), iter_log() before any step, also of SWEEP + 77 rows
                    (the later rounds of k_adopt_seed's copy); a refused adoption leaves the previous
                    plan's state_hash() unchanged
  law a             adopt(the single row `initial`) + step(k) is begin(initial) + step(k), bit for bit
                    (tree, regions, unexplored, rng; iter_log one iteration later), k = 1, 3, 8, four
                    scenarios, both step forms: through begin()'s side this ties adopted runs to the oracle
  law b             a multi-row adoption (the oracle's own tree after 6 iterations) gives the same
                    bytes on the one-launch and the two-launch form after 8 further iterations, and
                    the same state_hash() on two fresh handles
  law c             f64_model.audit_run over the adopted planners of law b, and over base's tree against
                    another obstacle list, cap 0.5 %; the measured shares are in test_law_c_float64_model
  law d             a 300-row chain adopted with the frontier at its last row: the tree passes take the
                    adopted depth into their bound
  the loop closed   demo seeds 1-3: plan, block the path, recheck, replan(alive=True), run to the end
"""
import ctypes

import numpy as np
import pytest

import f64_model
import tree_adopt_cases as ac
import tree_adopt_model as model
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL
from scenarios import SCENARIOS, make_oracle

pytestmark = pytest.mark.gpu

BY_NAME = {s.name: s for s in SCENARIOS}
FORMS = {"k_step": None, "two-launch": "0"}
R1_KEYS = ("R1", "R1Avail", "R1Valid", "R1Invalid")
SBMP_ERR_INVALID_ARGUMENT, SBMP_ERR_STATE = 1, 5


def u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def set_form(monkeypatch, form, sc=None):
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (sc.env.items() if sc else ()):
        monkeypatch.setenv(k, v)
    if FORMS[form] is not None:
        monkeypatch.setenv("SBMP_STEP", FORMS[form])


def planner(sc, **over):
    from cudasbmp_amd import KGMT
    cfg, extra = sc.config()
    cfg.update(over)
    return KGMT(**cfg, **extra)


def boxes_of(obs):
    from cudasbmp_amd import DeviceBuffer
    return DeviceBuffer(obs) if len(obs) else None


def same_planner_state(a, b, label, hashes=False):
    """tree, regions (after the export's fold), unexplored and rng of two planners, bit for bit."""
    for name, x, y in zip(("samples", "parents", "costs"), a.tree(), b.tree()):
        assert np.array_equal(u32(x), u32(y)), f"{label}: tree {name}"
    ra, rb = a.regions(), b.regions()
    for k in ra:
        assert np.array_equal(u32(ra[k]), u32(rb[k])), f"{label}: regions {k}"
    for name, x, y in zip(("unexplored", "uParent"), a.unexplored(), b.unexplored()):
        assert np.array_equal(u32(x), u32(y)), f"{label}: {name}"
    assert np.array_equal(a.rng(), b.rng()), f"{label}: rng"
    if hashes:
        assert a.state_hash() == b.state_hash(), f"{label}: state_hash"


def model_regions(state, cfg, goal=None, frontier_from=0):
    """regions() right after an adoption, from the model's tables."""
    t = model.tables(state, cfg["width"], cfg["N"], cfg["n"], goal, frontier_from)
    nR2 = cfg["N"] ** 2 * cfg["n"] ** 2
    bits = ((t["R2bits"][:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int32).ravel()[:nR2]
    out = {k: t[k] for k in R1_KEYS}
    out.update(R1Score=np.ones(cfg["N"] ** 2, dtype=np.float32), R2Avail=bits,
               R2Valid=np.zeros(nR2, dtype=np.int32), R2Invalid=np.zeros(nR2, dtype=np.int32))
    return out, t["summary"]


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("cid", ac.CASE_IDS)
def test_kernels_are_the_model_and_the_twin(cid):
    from cudasbmp_amd import tree_adopt_tables
    c = ac.case(cid)
    kw = dict(c.grid, goal=c.goal, frontier_from=c.frontier_from)
    dev = tree_adopt_tables(c.state, device=True, **kw)
    model.same_tables(dev, c.model, label=f"{c.name} device vs model")
    model.same_tables(dev, tree_adopt_tables(c.state, device=False, **kw), label=f"{c.name} device vs twin")
    again = tree_adopt_tables(c.state, device=True, **kw)
    for k in model.R1_TABLES + ("R2bits",):
        assert dev[k].tobytes() == again[k].tobytes(), f"{c.name}: {k} differs between two calls"
    assert dev["summary"] == again["summary"]


def test_device_entry_refuses_what_the_twin_refuses():
    from cudasbmp_amd import SbmpError, tree_adopt_tables
    st = ac.random_rows(10, 1)
    for over in (dict(frontier_from=11), dict(N=17), dict(n=0), dict(width=0.0), dict(goal=(np.nan, 1.0, 0.5))):
        with pytest.raises(SbmpError) as e:
            tree_adopt_tables(st, **dict(dict(width=20.0, height=20.0, N=16, n=8), **over))
        assert e.value.status == SBMP_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the oracle's trees (law b, law c)
_GROWN = {}


def grown(name, iters=6):
    """The oracle's own tree of scenario `name` after `iters` iterations: (samples, parents, costs)
    of the R rows, and the first row of the last iteration.  Computed once, never changed."""
    if name not in _GROWN:
        o = make_oracle(BY_NAME[name], plan=False)
        for _ in range(iters):
            assert o.step()
        R = o.info()["treeSize"]
        s, p, c = o.tree()
        first = int(o.iter_logs()[-1][1])          # treeSizeBefore of the last iteration
        out = (s[:R].copy(), p[:R].copy(), c[:R].copy(), first)
        for a in out[:3]:
            a.setflags(write=False)
        _GROWN[name] = out
    return _GROWN[name]


def frontier_of(name, which):
    s, _, _, first = grown(name)
    return {"0": 0, "last": first, "R": len(s)}[which]


def adopt_grown(g, name, which, obs=None, sc=None):
    sc = sc or BY_NAME[name]
    s, p, c, _ = grown(name)
    obs = sc.obstacles() if obs is None else obs
    d_obs = boxes_of(obs)
    out = g.adopt(s, p, c, sc.goal7(), d_obs, len(obs), sc.seed, frontier_from=frontier_of(name, which), depth_bound=7)
    return out, d_obs


# ---------------------------------------------------------------- the planner right after adopt()
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("which", ["0", "last", "R"])
def test_adopt_then_read_before_any_step(which, form, monkeypatch):
    sc = BY_NAME["base"]
    set_form(monkeypatch, form, sc)
    g = planner(sc)
    out, _keep = adopt_grown(g, "base", which)
    assert g.path_info()["form"] == form
    s, p, c, _ = grown("base")
    R, f = len(s), frontier_of("base", which)
    cfg, _ = sc.config()
    want, summary = model_regions(s[:, :4], cfg, (sc.goal[0], sc.goal[1], cfg["goalThreshold"]), f)
    assert out == summary and out["goalRow"] == -1 and (out["treeSize"], out["gLo"]) == (R, f)
    got = g.regions()
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(u32(got[k]), u32(want[k])), f"regions {k}"
    ts, tp, tc = g.tree()
    assert np.array_equal(u32(ts[:R]), u32(s)) and np.array_equal(tp[:R], p) and np.array_equal(u32(tc[:R]), u32(c))
    assert not ts[R:].any() and (tp[R:] == -1).all() and not tc[R:].any()
    log = g.iter_log()
    assert log.tolist() == [[1, R, 0, 0, 0, 0, 0, R, -1]], log       # row 1 is the adoption: S = A = 0
    r = g.result()
    assert (r.iterations, r.treeSize, r.goalIndex, r.stalled) == (1, R, -1, 0)    # the adoption is no stall


def test_adopt_of_a_tree_past_one_sweep(monkeypatch):
    """SWEEP + 77 rows into a planner of 2 SWEEP slots: k_adopt_seed's copy into treeState, treeCtrl
    and treeParent goes round its grid-stride loop a second time (only the planner entry copies).
    Random rows inside the workspace, random lower parents, distinct costs, the frontier at the
    last 64 rows, a goal no row holds; tree() and regions() before any step."""
    from cudasbmp_amd import KGMT
    set_form(monkeypatch, "k_step")
    S = ac.SWEEP
    state, ctrl, parent, f = ac.planner_past_sweep()
    R = len(parent)
    assert R == S + 77 and f == R - 64
    cfg = dict(DEMO, maxTreeSize=2 * S, numIterations=3)
    far_goal = (-5.0, -5.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    g = KGMT(**cfg)
    out = g.adopt(state, parent, ctrl, far_goal, None, 0, 7, frontier_from=f)
    want, summary = model_regions(state, cfg, (far_goal[0], far_goal[1], cfg["goalThreshold"]), f)
    assert out == summary and (out["rows"], out["treeSize"], out["gLo"], out["goalRow"]) == (R, R, f, -1)
    assert (out["nonFinite"], out["outOfGrid"]) == (0, 0)
    ts, tp, tc = g.tree()
    assert len(tp) == 2 * S
    for name, got, src in (("state", ts[:R, :4], state), ("controls", ts[:R, 4:7], ctrl[:, :3]), ("cost", tc[:R], ctrl[:, 3])):
        bad = np.flatnonzero((u32(got) != u32(src)).reshape(R, -1).any(axis=1))
        assert len(bad) == 0, f"{name}: {len(bad)} rows differ, first {bad[:8].tolist()} ({(bad >= S).sum()} at or past SWEEP)"
    bad = np.flatnonzero(tp[:R] != parent)
    assert len(bad) == 0, f"parent: {len(bad)} rows differ, first {bad[:8].tolist()}"
    assert not ts[R:].any() and (tp[R:] == -1).all() and not tc[R:].any()
    got = g.regions()
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(u32(got[k]), u32(want[k])), f"regions {k}"
    assert want["R1"].sum() == R and want["R2Avail"].all()
    assert g.iter_log().tolist() == [[1, R, 0, 0, 0, 0, 0, R, -1]]
    r = g.result()
    assert (r.iterations, r.treeSize, r.goalIndex, r.stalled) == (1, R, -1, 0)


def test_refused_adoption_leaves_the_previous_plan(monkeypatch):
    from cudasbmp_amd import SbmpError
    sc = BY_NAME["base"]
    set_form(monkeypatch, "k_step", sc)
    g = planner(sc, maxTreeSize=4096)
    obs = sc.obstacles()
    d_obs = boxes_of(obs)
    g.begin(sc.initial7(), sc.goal7(), d_obs, len(obs), sc.seed)
    g.step(2)
    before = g.state_hash()
    tree_before = [a.copy() for a in g.tree()]
    s, p, c, _ = grown("base")
    small = (s[:100].copy(), p[:100].copy(), c[:100].copy())
    nan_frontier = small[0].copy()
    nan_frontier[60, 2] = np.nan
    goal_nan = (np.nan,) + sc.goal7()[1:]
    refused = [
        (s, p, c, sc.goal7(), {}),                                         # R > M
        (*small, sc.goal7(), dict(frontier_from=-1)),
        (*small, sc.goal7(), dict(frontier_from=101)),
        (nan_frontier, small[1], small[2], sc.goal7(), dict(frontier_from=50)),   # D15 extended
        (*small, goal_nan, {}),
    ]
    for ss, pp, cc, goal, kw in refused:
        with pytest.raises(SbmpError) as e:
            g.adopt(ss, pp, cc, goal, d_obs, len(obs), sc.seed, **kw)
        assert e.value.status == SBMP_ERR_INVALID_ARGUMENT, kw
        assert g.state_hash() == before
    for x, y in zip(tree_before, g.tree()):
        assert np.array_equal(u32(x), u32(y))
    g.step(1)                                                              # and the plan goes on
    assert len(g.iter_log()) >= 2
    # a non-finite row below the frontier is adopted as stored
    out = g.adopt(nan_frontier, small[1], small[2], sc.goal7(), d_obs, len(obs), sc.seed, frontier_from=61)
    assert out["nonFinite"] == 1 and out["frontierNonFinite"] == 0
    assert np.array_equal(u32(g.tree()[0][:100]), u32(nan_frontier))


# ---------------------------------------------------------------- law a
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["base", "A-12x30-car-lds", "A-17.3x20-car-grid", "A-30x12-point-registers"])
def test_law_a_bit_exact_continuation(name, form, k, monkeypatch):
    sc = BY_NAME[name]
    set_form(monkeypatch, form, sc)
    obs = sc.obstacles()
    d_obs = boxes_of(obs)
    a, b = planner(sc), planner(sc)
    b.begin(sc.initial7(), sc.goal7(), d_obs, len(obs), sc.seed)
    root = np.array([sc.initial7()], dtype=np.float32)
    out = a.adopt(root, np.array([-1], dtype=np.int32), np.zeros(1, dtype=np.float32), sc.goal7(), d_obs, len(obs), sc.seed)
    assert (out["treeSize"], out["gLo"], out["goalRow"]) == (1, 0, -1)
    assert a.path_info() == b.path_info() and a.path_info()["form"] == form
    same_planner_state(a, b, f"{name} {form} before any step")
    a.step(k)
    b.step(k)
    same_planner_state(a, b, f"{name} {form} k={k}")
    la, lb = a.iter_log(), b.iter_log()
    assert len(lb) == k and len(la) == k + 1 and lb[:, 5].sum() > 0
    assert la[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, -1]
    shifted = la[1:].copy()
    shifted[:, 0] -= 1
    assert np.array_equal(shifted, lb), f"{name} {form}: iter_log one iteration later"


# ---------------------------------------------------------------- law b
@pytest.mark.parametrize("which", ["0", "last", "R"])
@pytest.mark.parametrize("name", ["base", "C-L2"])
def test_law_b_cross_form_agreement(name, which, monkeypatch):
    sc = BY_NAME[name]
    made = {}
    for label, form in (("one", "k_step"), ("two", "two-launch"), ("fresh", "k_step")):
        set_form(monkeypatch, form, sc)
        g = planner(sc, numIterations=10)
        _, keep = adopt_grown(g, name, which, sc=sc)
        assert g.path_info()["form"] == form
        g.step(8)
        made[label] = (g, keep)
    one, two, fresh = (made[k][0] for k in ("one", "two", "fresh"))
    same_planner_state(one, two, f"{name} frontier {which}: one launch vs two")
    assert np.array_equal(one.iter_log(), two.iter_log())
    assert one.state_hash() == fresh.state_hash()
    log = one.iter_log()
    R = len(grown(name)[0])
    assert len(log) == 9 and log[1][1] == R
    assert (log[1:, 5].sum() > 0) == (which != "R")                         # an empty frontier is D7's no-op loop
    if which != "R":
        assert log[-1][7] > R


# ---------------------------------------------------------------- law c
LAW_C = [("base", "0", None), ("base", "last", None), ("base", "R", None), ("C-L2", "0", None), ("C-L2", "last", None),
         ("C-L2", "R", None), ("base", "0", "E-7boxes-8steps")]


@pytest.mark.parametrize("name, which, other", LAW_C)
def test_law_c_float64_model(name, which, other, monkeypatch):
    """Every check of f64_model.audit_run, cap 0.5 % of borderline + edge children, 4 iterations after
    the adoption.  Measured on an MI355X (children; borderline share; edge share; worst err / bound):
        base, frontier 0              62,899   0.0159 %   0.0095 %   0.971
        base, last iteration's rows   63,680   0.0251 %   0.0016 %   0.983
        base, frontier R                   0   (D7's no-op loop: 4 iterations, nothing drawn)
        C-L2, frontier 0              64,971   0.0108 %   0.0169 %   0.977
        C-L2, last iteration's rows   48,796   0.0061 %   0         0.979
        C-L2, frontier R                   0
        base against E-7boxes-8steps  62,416   0.0224 %   0.0080 %   0.979
    The lottery lies within 2.2 sigma of its mean in every run."""
    sc = BY_NAME[name]
    set_form(monkeypatch, "k_step", sc)
    g = planner(sc)
    obs = BY_NAME[other].obstacles() if other else sc.obstacles()
    _, _keep = adopt_grown(g, name, which, obs=obs, sc=sc)
    cfg, extra = sc.config()
    st = f64_model.audit_run(g, cfg, obs, extra.get("agent", "car"), 4, cap=0.005, label=f"{name}/{which}/{other}")
    print(name, which, other, {k: (round(v, 6) if isinstance(v, float) else v) for k, v in st.items()})
    assert st["iterations"] >= 3
    if which != "R":
        assert st["children"] >= 16384 and st["state_rows"] > 0 and st["accepted"] > 0
    else:
        assert st["children"] == 0


# ---------------------------------------------------------------- law d
def chain(rows=300):
    st = np.zeros((rows, 4), dtype=np.float32)
    st[:, 0] = np.linspace(1.0, 16.0, rows)
    st[:, 1] = 13.0
    st[:, 3] = 0.5
    ctrl = np.zeros((rows, 4), dtype=np.float32)
    ctrl[:, 2] = 0.1
    ctrl[:, 3] = np.cumsum(ctrl[:, 2]) - np.float32(0.1)
    return st, np.arange(-1, rows - 1, dtype=np.int32), ctrl


@pytest.mark.parametrize("depth_bound", [0, 300])
def test_law_d_depth(depth_bound, monkeypatch):
    """A 300-row chain with the frontier at its last row, 3 iterations: the newest rows lie 301 and
    more rows deep.  With depth_bound() of kgmt_planner.h reverted to the old values, k_path_walk's
    bound is numIterations + 2 = 14 rows and the paths come back SBMP_PATH_DEEP, so the first
    assertions fail.  extract(root=0) would still keep every row: nothing on this tree is dead, and
    too few pointer-jumping passes can only miss a dead ancestor; it is held here all the same,
    but it does not detect that regression.  Checked on a scratch build with depth_bound() reverted: every
    one of the 2,038 newest paths came back with status 3 (SBMP_PATH_DEEP) and the test failed at the
    first assertion, for both depth_bound values; the extract half was not reached there."""
    from cudasbmp_amd import KGMT
    from cudasbmp_amd._native import SBMP_PATH_OK
    set_form(monkeypatch, "k_step")
    g = KGMT(**dict(DEMO, numIterations=12, goalThreshold=0.0), samplesPerIteration=4096, batchRule="fill")
    st, par, ctrl = chain()
    out = g.adopt(st, par, ctrl, DEMO_GOAL, None, 0, 3, frontier_from=299, depth_bound=depth_bound)
    assert (out["treeSize"], out["gLo"]) == (300, 299)
    g.step(3)
    R = g.result().treeSize
    log = g.iter_log()
    assert len(log) == 4 and R > 300 + 8
    newest = np.arange(int(log[-1][1]), R, dtype=np.int32)
    paths = g.solution_paths(newest)
    assert (paths["status"] == SBMP_PATH_OK).all() and (paths["lengths"] >= 301).all()
    assert paths["lengths"].max() >= 302
    ex = g.extract(root=0)
    assert ex["summary"]["kept"] == R and ex["summary"]["detached"] == 0
    rows, _, _ = g.solution_path(int(newest[-1]))
    assert len(rows) == paths["lengths"][-1] and rows[0] == 0


# ---------------------------------------------------------------- the loop closed
def outside_every_box(steps, boxes):
    x, y = steps[..., 0].ravel().astype(np.float64), steps[..., 1].ravel().astype(np.float64)
    z = np.zeros_like(x)
    hit, _, _ = f64_model._as_boxes(boxes).hits(x, x, y, y, z, z)
    return not hit.any()


def later_frontier(kept, M):
    """A frontier the reference batch rule can serve: k = floor(room / nG) = 4 children per parent."""
    return max(0, kept - max(1, (M - kept) // 4))


def test_the_loop_closed(obstacles):
    """Demo seeds 1-3: plan, a box on the solution path's middle row, recheck, replan(alive=True) with
    the frontier at the newest rows the room left can serve, run to the end.  A seed whose alive rows
    still hold a goal row ends at the adoption; the others must grow, and at least one does."""
    from cudasbmp_amd import KGMT, DeviceBuffer
    M = DEMO["maxTreeSize"]
    d_obs = DeviceBuffer(obstacles)
    far_goal = (-5.0, -5.0, 0.0, 0.0, 0.0, 0.0, 0.0)       # no row of the workspace lies within 0.5 of it
    grew = []
    for seed in (1, 2, 3):
        g = KGMT(**DEMO)
        r = g.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=seed)
        assert r.goalIndex > 0, "demo seeds 1-3 solve"
        rows, samples, costs = g.solution_path()
        mid = samples[len(rows) // 2]
        box = np.array([[mid[0] - 0.3, mid[1] - 0.3, mid[0] + 0.3, mid[1] + 0.3]], dtype=np.float32)
        new = np.concatenate([obstacles, box]).astype(np.float32)
        d_new = DeviceBuffer(new)
        _, chk = g.recheck(new)
        assert chk["blocked"] > 0 and chk["alive"] < chk["rows"]
        f = later_frontier(chk["alive"], M)
        out = g.replan(DEMO_GOAL, d_new, len(new), seed, alive=True, frontier_from=f)
        assert out["treeSize"] == chk["alive"] and out["gLo"] == f
        while g.step(8):
            pass
        res = g.result()
        log = g.iter_log()
        print(f"seed {seed}: adopted {out['treeSize']} of {chk['rows']} rows, frontier from {f}, goalRow {out['goalRow']}, "
              f"solved {res.goalIndex >= 0} after {res.iterations - 1} iterations, {res.treeSize} rows")
        if out["goalRow"] >= 0:
            assert (res.goalIndex, res.treeSize, len(log)) == (out["goalRow"], out["treeSize"], 1)
        else:
            assert res.treeSize > out["treeSize"] and len(log) >= 2 and log[1:, 6].sum() > 0
        grew.append(res.treeSize > out["treeSize"])
        _, final = g.recheck(new)
        assert final["rows"] == min(res.treeSize, M)
        assert (final["blocked"], final["stale"], final["orphan"]) == (0, 0, 0), final
        if res.goalIndex >= 0:
            tr = g.trajectories([res.goalIndex])
            assert tr["status"][0] == 0 and outside_every_box(tr["steps"][1:], new)
        # re-rooting: the new root keeps its stored cost, and the subtree grows on (towards a goal it cannot hold)
        for r_ in (int(rows[1]), int(rows[len(rows) // 2]), int(rows[-2])):
            g.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=seed)
            stored = g.tree()[2][r_].copy()
            want = g.extract(root=r_)
            kept = want["summary"]["kept"]
            assert kept >= 2                                    # r_ and, below it, the goal row
            out = g.replan(far_goal, d_obs, len(obstacles), seed, root=r_, frontier_from=later_frontier(kept, M))
            assert out["treeSize"] == kept and out["goalRow"] == -1
            s2, p2, c2 = g.tree()
            assert u32(c2[:1])[0] == u32(stored.reshape(1))[0] and p2[0] == -1
            assert np.array_equal(u32(s2[:kept, :4]), u32(want["state"]))
            g.step(2)
            log = g.iter_log()
            assert len(log) >= 2 and log[1:, 6].sum() > 0 and g.result().treeSize > kept
    assert any(grew), "no seed inserted a row after replan(alive=True)"


# ---------------------------------------------------------------- answers that are not errors
def test_an_adopted_goal_row_ends_the_plan_at_once(obstacles, monkeypatch):
    from cudasbmp_amd import KGMT, DeviceBuffer
    d_obs = DeviceBuffer(obstacles)
    donor = KGMT(**DEMO)
    r = donor.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=1)
    s, p, c = (a[:r.treeSize] for a in donor.tree())
    inside = np.flatnonzero(model.in_goal(s[:, 0], s[:, 1], DEMO_GOAL[:2] + (DEMO["goalThreshold"],)))
    assert len(inside) >= 1 and inside[0] == r.goalIndex
    # more rows of the disc, above the lowest: the lowest wins
    s = np.concatenate([s, s[inside[:1]], s[inside[:1]]])
    p = np.concatenate([p, p[inside[:1]], p[inside[:1]]])
    c = np.concatenate([c, c[inside[:1]], c[inside[:1]]])
    for form in FORMS:
        set_form(monkeypatch, form)
        g = KGMT(**DEMO)
        out = g.adopt(s, p, c, DEMO_GOAL, d_obs, len(obstacles), 1)
        assert out["goalRow"] == inside[0]
        assert g.step(1) is False
        res = g.result()
        assert (res.goalIndex, res.iterations, res.treeSize) == (inside[0], 1, len(s))
        assert u32(np.float32(res.costToGoal).reshape(1))[0] == u32(c[inside[:1]])[0]
        assert g.iter_log().tolist() == [[1, len(s), 0, 0, 0, 0, 0, len(s), inside[0]]]
        assert g.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=1).goalIndex == r.goalIndex


@pytest.mark.parametrize("form", list(FORMS))
def test_a_full_tree_runs_no_iteration(form, monkeypatch):
    from cudasbmp_amd import KGMT
    set_form(monkeypatch, form)
    s, p, c, _ = grown("base")
    R = 2000
    g = KGMT(**dict(DEMO, maxTreeSize=R, goalThreshold=0.0), samplesPerIteration=1024, batchRule="fill")
    out = g.adopt(s[:R], p[:R], c[:R], DEMO_GOAL, None, 0, 5)
    assert out["treeSize"] == R
    assert g.step(3) is False
    res = g.result()
    assert (res.iterations, res.treeSize, res.goalIndex) == (1, R, -1)
    assert np.array_equal(u32(g.tree()[0]), u32(s[:R]))


@pytest.mark.parametrize("form", list(FORMS))
def test_a_planner_without_iterations_refuses_and_one_iteration_adopts(form, monkeypatch):
    """The adoption is iteration 1 and plans iteration 2, so ctrl[2] must exist: numIterations = 0
    (two control blocks) is refused with SBMP_ERR_STATE before anything is touched; numIterations = 1
    adopts and runs nothing."""
    from cudasbmp_amd import KGMT, SbmpError
    set_form(monkeypatch, form)
    s, p, c, _ = grown("base")
    R = 500
    kw = dict(samplesPerIteration=1024, batchRule="fill")
    g0 = KGMT(**dict(DEMO, numIterations=0, goalThreshold=0.0), **kw)
    g0.begin(DEMO_INITIAL, DEMO_GOAL, None, 0, 1)
    before = g0.state_hash()
    for call in (lambda: g0.adopt(s[:R], p[:R], c[:R], DEMO_GOAL, None, 0, 5), lambda: g0.replan(DEMO_GOAL, None, 0, 5)):
        with pytest.raises(SbmpError) as e:
            call()
        assert e.value.status == SBMP_ERR_STATE and "numIterations" in str(e.value)
    assert g0.state_hash() == before and g0.step(1) is False
    g1 = KGMT(**dict(DEMO, numIterations=1, goalThreshold=0.0), **kw)
    out = g1.adopt(s[:R], p[:R], c[:R], DEMO_GOAL, None, 0, 5, frontier_from=400)
    assert out["treeSize"] == R
    assert g1.step(3) is False
    res = g1.result()
    assert (res.iterations, res.treeSize, res.goalIndex, res.stalled) == (1, R, -1, 0)
    assert g1.iter_log().tolist() == [[1, R, 0, 0, 0, 0, 0, R, -1]]
    assert np.array_equal(u32(g1.tree()[0][:R]), u32(s[:R]))


def test_out_of_scope_handles_say_so(obstacles):
    from cudasbmp_amd import KGMT, KGMTBatch, DeviceBuffer, SbmpError
    from cudasbmp_amd import _native as nat
    d_obs = DeviceBuffer(obstacles)
    root = np.array([DEMO_INITIAL], dtype=np.float32)
    one = (root, np.array([-1], dtype=np.int32), np.zeros(1, dtype=np.float32))
    uid = (ctypes.c_uint8 * nat.SBMP_COMM_ID_BYTES)()
    nat.call("sbmp_comm_get_unique_id", uid)
    batch = KGMTBatch(2, **DEMO)
    handles = {"a sharded rank": KGMT(**DEMO, _sharded=(bytes(uid), 1, 0)), "a local shard group": KGMT(**DEMO, _local_group=2),
               "a batch member": batch[0]}
    batch.begin([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d_obs, len(obstacles), [1, 2])
    for what, g in handles.items():
        if what != "a batch member":
            g.begin(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), 1)
        for call in (lambda: g.adopt(*one, DEMO_GOAL, d_obs, len(obstacles), 1),
                     lambda: g.replan(DEMO_GOAL, d_obs, len(obstacles), 1)):
            with pytest.raises(SbmpError) as e:
                call()
            assert e.value.status == SBMP_ERR_STATE, what
            assert "single-rank" in str(e.value) or "batch member" in str(e.value), str(e.value)


def test_plan_adopt_plan_is_a_fresh_handle(obstacles):
    from cudasbmp_amd import KGMT, DeviceBuffer
    d_obs = DeviceBuffer(obstacles)
    g, fresh = KGMT(**DEMO), KGMT(**DEMO)
    g.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=2)
    s, p, c, _ = grown("base")
    g.adopt(s[:5000], p[:5000], c[:5000], DEMO_GOAL, d_obs, len(obstacles), 7, frontier_from=4000)
    g.step(5)
    third = g.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=3)
    want = fresh.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=3)
    assert (third.iterations, third.treeSize, third.goalIndex) == (want.iterations, want.treeSize, want.goalIndex)
    assert g.state_hash() == fresh.state_hash()
    same_planner_state(g, fresh, "plan, adopt, plan against a fresh handle")

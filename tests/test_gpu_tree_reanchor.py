"""GPU: a grown tree re-anchored on a measured state (k_reanchor_*; include/sbmp/tree_reanchor.h).

Step level: sbmp_tree_reanchor_batch on every case of tests/tree_reanchor_cases.py against the
model (tests/tree_reanchor_model.py: the CPU oracle's replay level by level + numpy) and against
the host twin, bit for bit; every obstacle form; two calls give the same bytes; a depth bound
below the longest chain is refused.  The table's cases of SWEEP + 77 rows (one sweep of the grid is
at most 524,288 rows; fewer resident workgroups only start the later rounds sooner) take init, jump,
hist, scatter and one level past their first round, and its rows-2047 .. 2049 and chain-2046 .. 2048
cases stand either side of the 2,048 depth counters k_reanchor_hist keeps in LDS.  Three laws tie the new kernels to the ones that exist:
  a  s0 = the stored root and the planner's own boxes: every row recheck calls alive is alive
     here and keeps its stored state bit for bit (invariant I1)
  b  re-anchor on a displaced s0, extract the alive rows, re-check the result against the same
     boxes: every row is FREE (k_tree_recheck replays each row from its parent's new state)
  c  trace that result: every Euler state lies inside the workspace and outside every box
Planner level: KGMT.reanchor against the model over KGMT.tree() after plan(), between steps, with
the root on the solution path, on a batch member and on a local shard group; KGMT.replan_from on
demo seeds 1-3 run to the end.
"""
import ctypes

import numpy as np
import pytest

import tree_recheck_cases as tc
import tree_reanchor_cases as rc
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL
from scenarios import BASE, BASE_SEED
from tree_recheck_model import tree_arrays
from tree_reanchor_model import assert_same_reanchor, reanchor_model

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
SBMP_ERR_INVALID_ARGUMENT, SBMP_ERR_STATE = 1, 5
DEMO_PARAMS = dict(numDisc=DEMO["numDisc"], agentLength=DEMO["agentLength"], width=DEMO["width"], height=DEMO["height"],
                   agent="car")
MOVED = np.asarray(rc.MOVED, np.float32)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _split(kw):
    cfg = dict(DEMO)
    kw = dict(kw)
    extra = {k: kw.pop(k) for k in EXTRA_KEYS if k in kw}
    cfg.update(kw)
    return cfg, extra


def _mk(_local_group=0, **kw):
    from cudasbmp_amd import KGMT
    cfg, extra = _split(kw)
    return KGMT(**cfg, **extra, _local_group=_local_group)


def _dev(obs):
    from cudasbmp_amd import DeviceBuffer
    return DeviceBuffer(obs)


def device(c, **over):
    from cudasbmp_amd import tree_reanchor_batch
    kw = dict(c.params, depth_bound=c.bound)
    kw.update(over)
    return tree_reanchor_batch(c.state, c.ctrl, c.parent, c.s0, c.boxes, **kw)


def refused(c, **over):
    from cudasbmp_amd import SbmpError
    with pytest.raises(SbmpError) as e:
        device(c, **over)
    assert e.value.status == SBMP_ERR_INVALID_ARGUMENT
    return str(e.value)


def _check(c):
    if c.refused:
        assert "depthBound" in refused(c)
        return None
    dev = device(c)
    assert_same_reanchor(dev, c.model, label=f"{c.name} device vs model")
    assert_same_reanchor(device(c, device=False), c.model, label=f"{c.name} host vs model")
    return dev


# ---------------------------------------------------------------- step level
@pytest.mark.parametrize("build", [b for _, b in rc.CASES], ids=rc.CASE_IDS)
def test_device_matches_model_and_host(build):
    _check(build())


@pytest.mark.parametrize("variant, count", [("1", 8), ("2", 600), ("2", 9), ("4", 5), ("4", 600), ("5", 3000)],
                         ids=["lds-8", "lds4-600", "lds4-9", "grid-5", "grid-600", "global-3000"])
def test_forced_obstacle_forms(variant, count, monkeypatch):
    """SBMP_EXPAND_VARIANT as the planner reads it: the LDS forms below their thresholds, the grid
    at any count, the global loop where the planner would take it (the automatic choice, in the
    table above, is registers up to 8 boxes, LDS up to 2,048 and the grid beyond)."""
    monkeypatch.setenv("SBMP_EXPAND_VARIANT", variant)
    _check(rc.nan_case(5) if count == 5 else rc.boxes_case(count))


@pytest.mark.parametrize("variant", ["1", "2", "4", "5"])
def test_forced_forms_on_a_deep_tree(variant, monkeypatch):
    monkeypatch.setenv("SBMP_EXPAND_VARIANT", variant)
    _check(rc.grown(*tc.MAIN, "moved"))
    _check(rc.grown("point", 1.0, 13, "moved"))


@pytest.mark.parametrize("build", [lambda: rc.grown(*tc.MAIN, "moved"), lambda: rc.chain(257, "last", "same"),
                                   rc.far_parent, lambda: rc.boxes_case(3000), lambda: rc.star(rc.STAR_ROWS),
                                   rc.big_star, lambda: rc.recursive(0)],
                         ids=["grown", "chain", "far-parent", "grid", "star", "star-sweep+77", "recursive-sweep+77"])
def test_two_calls_give_identical_bytes(build):
    """The order of the rows inside a level is whatever the atomics give: no output byte depends on it."""
    c = build()
    a, b = device(c), device(c)
    for k in ("state", "alive", "status"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["summary"] == b["summary"]


def test_a_short_bound_is_refused_not_answered():
    """A chain of 9 rows with bound 4: two passes cover four of its eight edges.  Bounds that only
    look short (8 and 5 both give three passes, which cover the eight edges) are answered, rightly."""
    c = rc.chain(8, "last")
    assert "depthBound" in refused(c, depth_bound=4)
    assert "depthBound" in refused(c, depth_bound=2)
    assert "depthBound" in refused(c, depth_bound=1)
    for bound in (5, 8, 9, 16, 1 << 20):
        assert_same_reanchor(device(c, depth_bound=bound), c.model, label=f"bound {bound}")
    g = rc.grown(*tc.MAIN, "moved")
    assert "depthBound" in refused(g, depth_bound=8)        # 13 levels: three passes cover eight edges
    assert_same_reanchor(device(g, depth_bound=9), g.model, label="grown, bound 9: four passes")


@pytest.mark.parametrize("bad", list(rc.BAD_ROOTS), ids=list(rc.BAD_ROOTS))
def test_a_non_finite_root_is_refused(bad):
    c = rc.chain(8, "last")
    refused(rc.RCase(c.name, c.state, c.ctrl, c.parent, c.boxes, c.params, np.array(rc.BAD_ROOTS[bad], np.float32)))


def test_outputs_may_stay_away():
    """d_outState, d_alive and status are optional: the summary is the same without them."""
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    c = rc.grown(*tc.MAIN, "moved")
    devs = [_Dev(c.state), _Dev(c.ctrl), _Dev(c.parent), _Dev(c.boxes)]
    try:
        a = nat.TreeRecheckArgs()
        a.state, a.ctrl, a.parent, a.obstacles = (d.ptr for d in devs)
        a.rows, a.obstaclesCount, a.agent, a.numDisc = len(c.parent), len(c.boxes), nat.SBMP_AGENT_CAR, 10
        a.agentLength, a.width, a.height = 1.0, c.params["width"], c.params["height"]
        s = nat.TreeReanchor()
        s0 = np.ascontiguousarray(c.s0, np.float32)
        nat.call("sbmp_tree_reanchor_batch", ctypes.byref(a), s0.ctypes.data_as(ctypes.c_void_p), None, None, None,
                 ctypes.byref(s), None)
        assert {k: getattr(s, k) for k, _ in nat.TreeReanchor._fields_} == c.model[3]
    finally:
        for d in devs:
            d.close()


# ---------------------------------------------------------------- the three laws
LAW_CASES = [("grown-" + i, (lambda g=g: rc.grown(*g, "moved"))) for g, i in zip(tc.GROWN, tc.GROWN_IDS)]
LAW_CASES += [("far-parent", rc.far_parent), ("blocked", rc.blocked), ("wall", rc.wall),
              ("boxes-600", lambda: rc.boxes_case(600))]


def inside_and_outside(steps, boxes, width, height):
    """Every (x, y) of steps lies strictly inside the workspace and in no box's open interior."""
    x, y = steps[..., 0].ravel().astype(np.float64), steps[..., 1].ravel().astype(np.float64)
    if not ((x > 0).all() and (x < width).all() and (y > 0).all() and (y < height).all()):
        return False
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    b = b[~np.isnan(b).any(axis=1)]
    for i in range(0, len(x), 1 << 14):
        xs, ys = x[i:i + (1 << 14), None], y[i:i + (1 << 14), None]
        if ((xs > b[:, 0]) & (xs < b[:, 2]) & (ys > b[:, 1]) & (ys < b[:, 3])).any():
            return False
    return True


@pytest.mark.parametrize("build", [b for _, b in LAW_CASES], ids=[i for i, _ in LAW_CASES])
def test_laws_b_and_c_the_result_is_a_tree_of_the_planners_own(build):
    from cudasbmp_amd import tree_extract_batch, tree_recheck_batch, tree_trace_batch
    c = build()
    got = device(c)
    kept = tree_extract_batch(got["state"], c.ctrl, c.parent, keep=got["alive"])
    K = kept["summary"]["kept"]
    assert K == got["summary"]["alive"] >= 2
    assert np.array_equal(u32(kept["state"][0]), u32(c.s0))
    # law b: k_tree_recheck replays every row of the result from its parent's new state
    status, s = tree_recheck_batch(kept["state"], kept["ctrl"], kept["parent"], c.boxes, **c.params)
    assert s == dict(rows=K, alive=K, blocked=0, stale=0, orphan=0, cut=0, firstDead=-1), s
    assert not status.any()
    # law c: the Euler states of every edge of the result
    p = c.params
    steps, st = tree_trace_batch(kept["state"], kept["ctrl"], kept["parent"], numDisc=p["numDisc"],
                                 agentLength=p["agentLength"], agent=p["agent"])
    assert not st.any()
    assert inside_and_outside(np.asarray(steps)[1:], c.boxes, p["width"], p["height"])


def _grown_planner(obstacles, **kw):
    g = _mk(**dict(BASE, **kw))
    g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=BASE_SEED)
    s, p, c = g.tree()
    return g, tree_arrays(s, p, c, g.result().treeSize)


def test_law_a_the_stored_root_gives_the_stored_tree(obstacles):
    from cudasbmp_amd import tree_reanchor_batch
    g, (state, ctrl, parent) = _grown_planner(obstacles)
    status, chk = g.recheck(obstacles)
    alive = status == 0
    assert chk["alive"] == alive.sum() >= 1000
    got = tree_reanchor_batch(state, ctrl, parent, state[0], obstacles, **DEMO_PARAMS)
    assert got["alive"][alive].all()
    assert np.array_equal(u32(got["state"][alive]), u32(state[alive]))
    own = g.reanchor(state[0], root=0, obstacles=obstacles)
    assert own["alive"][alive].all() and np.array_equal(u32(own["state"][alive]), u32(state[alive]))


# ---------------------------------------------------------------- planner level
def _model_of_planner(g, root, s0, boxes, params=DEMO_PARAMS):
    """The model over extract(root) of the planner's own tree (the extraction has tests of its own)."""
    ex = g.extract(root=root)
    return ex, reanchor_model(ex["state"], ex["ctrl"], ex["parent"], s0, boxes, **params)


def _same_as_model(got, ex, want, label):
    assert_same_reanchor(got, want, label=label)
    for k in ("ctrl", "parent", "origin"):
        assert np.array_equal(got[k].view(np.uint32), ex[k].view(np.uint32)), f"{label}: {k}"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reanchor_of_the_demo_plan(seed, obstacles):
    g = _mk()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0
    h = g.state_hash()
    rows, samples, _ = g.solution_path()
    for root in (0, int(rows[1]), int(rows[len(rows) // 2])):
        s0 = (g.tree()[0][root, :4] + MOVED).astype(np.float32)
        ex, want = _model_of_planner(g, root, s0, obstacles)
        got = g.reanchor(s0, root=root, obstacles=obstacles)
        _same_as_model(got, ex, want, f"seed {seed} root {root}")
        assert got["summary"]["rows"] == ex["summary"]["kept"]
    got = g.reanchor(s0, root=root, obstacles=_dev(obstacles), obstaclesCount=len(obstacles))   # the device-pointer form
    _same_as_model(got, ex, want, f"seed {seed} device pointer")
    assert g.state_hash() == h


def test_reanchor_between_steps_changes_nothing(obstacles):
    def run(reanchor):
        g = _mk(**BASE)
        g.begin(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), BASE_SEED)
        seen = []
        for _ in range(2):
            g.step(3)
            if reanchor:
                s0 = (np.asarray(DEMO_INITIAL[:4], np.float32) + MOVED).astype(np.float32)
                ex, want = _model_of_planner(g, 0, s0, obstacles)
                got = g.reanchor(s0, obstacles=obstacles)
                _same_as_model(got, ex, want, f"after {3 * (len(seen) + 1)} iterations")
                seen.append(got["summary"])
        while g.step(4):
            pass
        return g, seen

    g0, _ = run(False)
    g1, seen = run(True)
    assert seen[0]["rows"] < seen[1]["rows"] and seen[0]["levels"] < seen[1]["levels"]
    assert g1.state_hash() == g0.state_hash()
    for x, y in zip(g1.tree(), g0.tree()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_local_group_and_batch_member_answer_as_one_planner(obstacles):
    from cudasbmp_amd import KGMTBatch
    d = _dev(obstacles)
    s0 = (np.asarray(DEMO_INITIAL[:4], np.float32) + MOVED).astype(np.float32)
    single, _ = _grown_planner(obstacles)
    ex, want = _model_of_planner(single, 0, s0, obstacles)
    _same_as_model(single.reanchor(s0, obstacles=obstacles), ex, want, "single")
    group = _mk(_local_group=2, **BASE)
    group.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    _same_as_model(group.reanchor(s0, obstacles=obstacles), ex, want, "local group of 2")
    cfg, extra = _split(BASE)
    b = KGMTBatch(2, **cfg, **extra)
    b.plan([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d, len(obstacles), [BASE_SEED + 1, BASE_SEED])
    _same_as_model(b[1].reanchor(s0, obstacles=obstacles), ex, want, "batch member 1")
    ex0, want0 = _model_of_planner(b[0], 0, s0, obstacles)
    _same_as_model(b[0].reanchor(s0, obstacles=obstacles), ex0, want0, "batch member 0")


def later_frontier(kept, M):
    """A frontier the reference batch rule can serve: k = floor(room / nG) = 4 children per parent."""
    return max(0, kept - max(1, (M - kept) // 4))


def test_replan_from_a_displaced_state(obstacles):
    """Demo seeds 1-3: plan, drive to a row of the solution path, measure a state a tracking error
    off it, replan_from there towards a goal no row can hold, run to the end.  The adopted tree is
    the model's alive rows with their new states, row 0 is the measured state bit for bit, rows
    are inserted after the adoption, and the final tree re-checks without a dead row."""
    from cudasbmp_amd import SbmpError
    M = DEMO["maxTreeSize"]
    d_obs = _dev(obstacles)
    far_goal = (-5.0, -5.0, 0.0, 0.0, 0.0, 0.0, 0.0)       # no row of the workspace lies within 0.5 of it
    for seed in (1, 2, 3):
        g = _mk()
        r = g.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), seed=seed)
        assert r.goalIndex > 0, "demo seeds 1-3 solve"
        rows, _, _ = g.solution_path()
        root = int(rows[len(rows) // 2])
        s0 = (g.tree()[0][root, :4] + MOVED).astype(np.float32)
        ex, (wout, walive, _, wsum) = _model_of_planner(g, root, s0, obstacles)
        assert wsum["alive"] >= 2
        h = g.state_hash()
        for bad in ((np.nan, 1.0, 0.0, 0.0), (1.0, np.inf, 0.0, 0.0)):
            with pytest.raises(SbmpError) as e:
                g.replan_from(bad, far_goal, d_obs, len(obstacles), seed, root=root)
            assert e.value.status == SBMP_ERR_INVALID_ARGUMENT
        for kw in (dict(root=root, frontier_from=wsum["alive"] + 1), dict(root=root, frontier_from=-1),
                   dict(root=min(r.treeSize, M))):
            with pytest.raises(SbmpError) as e:
                g.replan_from(s0, far_goal, d_obs, len(obstacles), seed, **kw)
            assert e.value.status == SBMP_ERR_INVALID_ARGUMENT, kw
        assert g.state_hash() == h                                  # a refused call leaves the plan as it was
        f = later_frontier(wsum["alive"], M)
        out = g.replan_from(s0, far_goal, d_obs, len(obstacles), seed, root=root, frontier_from=f)
        assert out["reanchor"] == wsum
        K = wsum["alive"]
        assert (out["adopt"]["rows"], out["adopt"]["treeSize"], out["adopt"]["gLo"], out["adopt"]["goalRow"]) == (K, K, f, -1)
        s2, p2, c2 = g.tree()
        assert np.array_equal(u32(s2[0, :4]), u32(s0)) and p2[0] == -1
        assert np.array_equal(u32(s2[:K, :4]), u32(wout[walive]))
        assert np.array_equal(u32(c2[:K]), u32(ex["ctrl"][walive, 3]))      # costs stay as stored
        while g.step(8):
            pass
        res = g.result()
        print(f"seed {seed}: root {root}, {wsum}, frontier from {f}, {res.treeSize} rows after {res.iterations - 1} iterations")
        assert res.treeSize > K
        _, final = g.recheck(obstacles)
        assert final["rows"] == min(res.treeSize, M)
        assert (final["blocked"], final["stale"], final["orphan"], final["cut"]) == (0, 0, 0, 0), final
        assert np.array_equal(u32(g.tree()[0][0, :4]), u32(s0))


def test_out_of_scope_handles_say_so(obstacles):
    from cudasbmp_amd import KGMT, KGMTBatch, SbmpError
    from cudasbmp_amd import _native as nat
    d_obs = _dev(obstacles)
    uid = (ctypes.c_uint8 * nat.SBMP_COMM_ID_BYTES)()
    nat.call("sbmp_comm_get_unique_id", uid)
    batch = KGMTBatch(2, **DEMO)
    handles = {"a sharded rank": KGMT(**DEMO, _sharded=(bytes(uid), 1, 0)), "a local shard group": KGMT(**DEMO, _local_group=2),
               "a batch member": batch[0]}
    batch.begin([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d_obs, len(obstacles), [1, 2])
    for what, g in handles.items():
        if what != "a batch member":
            g.begin(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), 1)
        with pytest.raises(SbmpError) as e:
            g.replan_from(DEMO_INITIAL[:4], DEMO_GOAL, d_obs, len(obstacles), 1)
        assert e.value.status == SBMP_ERR_STATE, what
        assert "single-rank" in str(e.value) or "batch member" in str(e.value), str(e.value)
    g0 = _mk(numIterations=0)
    g0.begin(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obstacles), 1)
    with pytest.raises(SbmpError) as e:
        g0.replan_from(DEMO_INITIAL[:4], DEMO_GOAL, d_obs, len(obstacles), 1)
    assert e.value.status == SBMP_ERR_STATE and "numIterations" in str(e.value)


def test_state_errors_and_the_capacity_protocol(obstacles):
    from cudasbmp_amd import SbmpError
    from cudasbmp_amd import _native as nat
    g = _mk(**BASE)
    d = _dev(obstacles)
    s0 = np.ascontiguousarray(np.asarray(DEMO_INITIAL[:4], np.float32) + MOVED, np.float32)
    with pytest.raises(SbmpError) as e:
        g.reanchor(s0, obstacles=obstacles)
    assert e.value.status == SBMP_ERR_STATE                         # before the first begin()
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    g.step(4)
    L = nat.lib()
    p0 = s0.ctypes.data_as(ctypes.c_void_p)
    dp = ctypes.c_void_p(d.ptr)
    out = nat.TreeReanchor()
    n = len(obstacles)
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, dp, n, None, None, None, None, None, 0, ctypes.byref(out)) == 0
    R = out.rows                                                    # NULL / 0: the size, and the summary
    assert R == min(g.result().treeSize, g.M) and out.alive + out.blocked + out.orphan + out.cut == R and 2 <= out.levels <= 5
    small = np.zeros(R - 1, np.uint8)
    out2 = nat.TreeReanchor()
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, dp, n, None, None, None, None, small.ctypes.data_as(ctypes.c_void_p),
                                     R - 1, ctypes.byref(out2)) == SBMP_ERR_INVALID_ARGUMENT
    assert out2.rows == R                                           # set in every case
    exact = np.zeros(R, np.uint8)
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, dp, n, None, None, None, None, exact.ctypes.data_as(ctypes.c_void_p), R,
                                     ctypes.byref(out2)) == 0
    assert (exact == 0).sum() == out.alive
    assert L.sbmp_kgmt_reanchor_tree(g._h, R, p0, dp, n, None, None, None, None, None, 0, ctypes.byref(out2)) == 1
    assert L.sbmp_kgmt_reanchor_tree(g._h, -1, p0, dp, n, None, None, None, None, None, 0, ctypes.byref(out2)) == 1
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, None, dp, n, None, None, None, None, None, 0, ctypes.byref(out2)) == 1
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, None, n, None, None, None, None, None, 0, ctypes.byref(out2)) == 1
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, dp, -1, None, None, None, None, None, 0, ctypes.byref(out2)) == 1
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, dp, n, None, None, None, None, None, 0, None) == 1
    nan = np.array([np.nan, 1, 0, 0], np.float32)
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, nan.ctypes.data_as(ctypes.c_void_p), dp, n, None, None, None, None, None, 0,
                                     ctypes.byref(out2)) == 1
    assert L.sbmp_kgmt_reanchor_tree(g._h, 0, p0, None, 0, None, None, None, None, None, 0, ctypes.byref(out2)) == 0
    assert out2.rows == R and out2.alive >= out.alive               # an empty list: only the walls block

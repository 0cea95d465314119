"""GPU: the tree re-check (k_tree_recheck, k_tree_alive, k_tree_query_alive; include/sbmp/tree_recheck.h).

Step level: sbmp_tree_recheck_batch on every case of tests/tree_recheck_cases.py against the
model (tests/tree_recheck_model.py: the CPU oracle's replay + numpy) and against the host twin,
byte for byte; row counts round the wave and workgroup sizes, and a star tree one row longer
than a full sweep of the grid (at most 8 workgroups of 256 rows per CU).  Planner level:
KGMT.recheck and KGMT.query_goals(alive=True) against the models over KGMT.tree(), after
plan(), between steps, on a local shard group and on a batch member.
"""
import numpy as np
import pytest

import tree_recheck_cases as tc
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, bits
from scenarios import BASE, BASE_SEED, demo_plus, random_boxes
from tree_query_model import assert_same_answers, model_of_rows
from tree_recheck_model import BLOCKED, FREE, assert_same_recheck, recheck_model, tree_arrays

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
SBMP_ERR_INVALID_ARGUMENT, SBMP_ERR_STATE = 1, 5
DEMO_PARAMS = dict(numDisc=DEMO["numDisc"], agentLength=DEMO["agentLength"], width=DEMO["width"], height=DEMO["height"],
                   agent="car")


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


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


def device(case, **kw):
    from cudasbmp_amd import tree_recheck_batch
    return tree_recheck_batch(case.state, case.ctrl, case.parent, case.boxes, **case.params, **kw)


def _check(case):
    status, summary, _ = case.model
    dev = device(case)
    assert_same_recheck(dev, (status, summary), label=f"{case.name} device vs model")
    assert_same_recheck(dev, device(case, device=False), label=f"{case.name} device vs host")
    return dev


def _model_of_tree(g, boxes):
    s, p, c = g.tree()
    state, ctrl, parent = tree_arrays(s, p, c, g.result().treeSize)
    return recheck_model(state, ctrl, parent, boxes, **DEMO_PARAMS), (state, ctrl, parent)


def _alive_answers(state, ctrl, alive, goals):
    """tests/tree_query_model.py over the alive rows only, row numbers mapped back to the tree's."""
    return model_of_rows(state, ctrl, goals, alive)


# ---------------------------------------------------------------- step level
@pytest.mark.parametrize("build", [b for _, b in tc.CPU_CASES], ids=tc.CPU_IDS)
def test_device_matches_model_and_host(build):
    _check(build())


@pytest.mark.parametrize("rows", tc.ROW_COUNTS)
def test_row_counts_round_the_wave_and_the_workgroup(rows):
    _check(tc.rows_case(rows))


def test_one_row_more_than_a_full_grid_sweep():
    # at most 8 workgroups of 256 rows on each of an MI355X's 256 CUs: the last row is the one
    # row of the grid-stride loops' second round (fewer resident workgroups only start it sooner)
    case = tc.star_case(256 * 8 * 256 + 1)
    status, summary = _check(case)
    assert summary["cut"] == 0 and summary["blocked"] >= 1 and summary["alive"] >= 2
    assert status[-1] in (FREE, BLOCKED)


@pytest.mark.parametrize("build", [lambda: tc.blocked(*tc.MAIN), lambda: tc.chain_case(257, "first"),
                                   lambda: tc.boxes_case(3000)], ids=["blocked", "chain", "grid"])
def test_two_launches_give_identical_bytes(build):
    case = build()
    a, b = device(case), device(case)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("variant, count", [("1", 8), ("2", 600), ("2", 9), ("4", 5), ("4", 600), ("5", 3000)],
                         ids=["lds-8", "lds4-600", "lds4-9", "grid-5", "grid-600", "global-3000"])
def test_forced_obstacle_forms(variant, count, monkeypatch):
    """SBMP_EXPAND_VARIANT as the planner reads it: the LDS forms below their thresholds, the grid
    at any count, the global loop where the planner would take it."""
    monkeypatch.setenv("SBMP_EXPAND_VARIANT", variant)
    _check(tc.boxes_case(count))


def test_depth_bound_sets_the_passes_not_the_answer():
    case = tc.chain_case(257, "first")
    for bound in (258, 300, 1 << 20):
        assert_same_recheck(device(case, depthBound=bound), case.model[:2], label=f"depthBound {bound}")


# ---------------------------------------------------------------- planner level
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recheck_of_the_demo_plan(seed, obstacles):
    g = _mk()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0
    R = min(r.treeSize, DEMO["maxTreeSize"])
    status, summary = g.recheck(obstacles)
    assert summary == dict(rows=R, alive=R, blocked=0, stale=0, orphan=0, cut=0, firstDead=-1)
    assert len(status) == R and not status.any()
    # one box on the row half way along the solution path
    rows, ps, _ = g.solution_path()
    mid = int(rows[len(rows) // 2])
    x, y = ps[len(rows) // 2, :2]
    boxes = demo_plus((x - 0.05, y - 0.05, x + 0.05, y + 0.05))
    (want, wsum, alive), (state, ctrl, parent) = _model_of_tree(g, boxes)
    assert want[mid] == BLOCKED and wsum["cut"] >= 1 and not alive[r.goalIndex]
    got = g.recheck(_dev(boxes), len(boxes))                      # the device-pointer form
    assert_same_recheck(got, (want, wsum), label=f"seed {seed}")
    goals = np.array([[DEMO_GOAL[0], DEMO_GOAL[1], 0.5], [5.0, 5.0, 0.5], [x, y, 1.0], [12.0, 3.0, 2.0], [9.0, 7.0, 0.5]],
                     np.float32)
    a = g.query_goals(goals, alive=True)
    assert_same_answers(a, _alive_answers(state, ctrl, alive, goals), label=f"seed {seed} alive")
    assert a["firstRow"][0] != r.goalIndex                        # the plan's own goal row is cut off
    seen = 0
    for best in a["bestRow"]:
        if best >= 0:
            path = g.solution_path(int(best))[0]
            assert alive[path].all() and path[-1] == best
            seen += 1
    assert seen >= 2
    assert_same_answers(g.query_goals(goals), model_of_rows(state, ctrl, goals), label="the unmasked query is unchanged")


ALIVE_GOAL_COUNTS = (1, 3, 4, 7, 8, 9, 13, 17)


def _lattice_goals(count):
    """The first `count` points of a 5 x 5 lattice of pitch 4 over the 20 x 20 workspace, the
    root's own point (5, 5) first.  Radii alternate: 1.5 (the root, always alive, lies inside
    goal 0) and 0.001 (no row comes that close to a lattice point)."""
    pts = [((5 + 4 * i) % 20, (5 + 4 * j) % 20) for j in range(5) for i in range(5)][:count]
    return np.array([[x, y, 1.5 if k % 2 == 0 else 0.001] for k, (x, y) in enumerate(pts)], np.float32)


@pytest.fixture(scope="module")
def rechecked_plan(obstacles):
    """One grown plan, re-checked against the other box list, and the model of that re-check."""
    g = _mk(**BASE)
    g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=BASE_SEED)
    other = random_boxes(600, 20.0, 20.0, 7, 0.3, 0.8)
    got = g.recheck(other)
    (want, wsum, alive), (state, ctrl, _) = _model_of_tree(g, other)
    assert_same_recheck(got, (want, wsum), label="the re-check under the masked queries")
    return g, state, ctrl, alive


@pytest.mark.parametrize("count", ALIVE_GOAL_COUNTS)
def test_masked_query_over_every_tile_of_the_ladder(count, rechecked_plan):
    """query_goals(alive=True) for goal counts that launch every tile of the masked query's
    ladder (8, 4, 1) alone, repeated and behind one another: 17 = 8 + 8 + 1, 13 = 8 + 4 + 1,
    7 = 4 + 1 + 1 + 1.  Field for field against the model over the alive rows.  Some goal has
    rows inside and, from two goals on (one goal cannot be both), some goal has none."""
    g, state, ctrl, alive = rechecked_plan
    assert alive.any() and not alive.all()                        # the mask is mixed
    goals = _lattice_goals(count)
    a = g.query_goals(goals, alive=True)
    print(f"{count} goals: count {a['count'].tolist()}")
    assert_same_answers(a, _alive_answers(state, ctrl, alive, goals), label=f"{count} goals alive")
    assert (a["count"] > 0).any()
    if count >= 2:
        assert (a["count"] == 0).any()


def test_recheck_between_steps_changes_nothing(obstacles):
    kw = dict(BASE)
    other = random_boxes(600, 20.0, 20.0, 7, 0.3, 0.8)

    def run(recheck):
        g = _mk(**kw)
        g.begin(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), BASE_SEED)
        seen = []
        for _ in range(2):
            g.step(3)
            if recheck:
                got = g.recheck(other)
                (want, wsum, _), _ = _model_of_tree(g, other)
                assert_same_recheck(got, (want, wsum), label=f"after {3 * (len(seen) + 1)} iterations")
                seen.append(got[1])
        while g.step(4):
            pass
        return g, seen

    g0, _ = run(False)
    g1, seen = run(True)
    assert seen[0]["rows"] < seen[1]["rows"] and seen[1]["blocked"] >= 1
    assert g1.state_hash() == g0.state_hash()
    for x, y in zip(g1.tree(), g0.tree()):
        assert np.array_equal(bits(x), bits(y))
    r0, r1 = g0.result(), g1.result()
    assert (r1.iterations, r1.treeSize, r1.accepted) == (r0.iterations, r0.treeSize, r0.accepted)


def test_a_long_list_leaves_the_plans_form_alone(obstacles):
    g = _mk(**BASE)
    g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=BASE_SEED)
    before, h = g.path_info(), g.state_hash()
    assert before["obstacle_form"] == "registers"
    boxes = random_boxes(3000, 20.0, 20.0, 11, 0.08, 0.5)
    got = g.recheck(boxes)
    (want, wsum, _), _ = _model_of_tree(g, boxes)
    assert_same_recheck(got, (want, wsum), label="3,000 boxes")
    assert wsum["blocked"] >= 1
    assert g.path_info() == before and g.state_hash() == h
    assert g.recheck(obstacles)[1]["alive"] == wsum["rows"]      # the plan's own list is still what it was


def test_local_group_and_batch_member_answer_as_one_planner(obstacles):
    from cudasbmp_amd import KGMTBatch
    kw = dict(BASE)
    d = _dev(obstacles)
    other = random_boxes(600, 20.0, 20.0, 7, 0.3, 0.8)
    goals = np.array([[DEMO_GOAL[0], DEMO_GOAL[1], 2.0], [5.0, 5.0, 0.5], [15.0, 15.0, 3.0]], np.float32)
    single = _mk(**kw)
    single.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    want = single.recheck(other)
    (ms, msum, alive), (state, ctrl, _) = _model_of_tree(single, other)
    assert_same_recheck(want, (ms, msum), label="single")
    qa = single.query_goals(goals, alive=True)
    assert_same_answers(qa, _alive_answers(state, ctrl, alive, goals), label="single alive")
    group = _mk(_local_group=2, **kw)
    group.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    assert_same_recheck(group.recheck(other), want, label="local group of 2")
    assert_same_answers(group.query_goals(goals, alive=True), qa, label="local group of 2 alive")
    cfg, extra = _split(kw)
    b = KGMTBatch(2, **cfg, **extra)
    b.plan([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d, len(obstacles), [BASE_SEED + 1, BASE_SEED])
    assert_same_recheck(b[1].recheck(other), want, label="batch member 1")
    assert_same_answers(b[1].query_goals(goals, alive=True), qa, label="batch member 1 alive")
    (m0, m0sum, _), _ = _model_of_tree(b[0], other)
    assert_same_recheck(b[0].recheck(other), (m0, m0sum), label="batch member 0")


def test_state_and_argument_errors(obstacles):
    import ctypes

    from cudasbmp_amd import SbmpError
    from cudasbmp_amd import _native as nat
    g = _mk(**BASE)
    d = _dev(obstacles)

    def status_of(f):
        with pytest.raises(SbmpError) as e:
            f()
        return e.value.status

    assert status_of(lambda: g.recheck(obstacles)) == SBMP_ERR_STATE                    # before the first begin()
    assert status_of(lambda: g.query_goals([[1.0, 1.0]], 0.5, alive=True)) == SBMP_ERR_STATE
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    g.step(3)
    assert status_of(lambda: g.query_goals([[1.0, 1.0]], 0.5, alive=True)) == SBMP_ERR_STATE   # no recheck yet
    out = nat.TreeRecheck()
    L = nat.lib()
    assert L.sbmp_kgmt_recheck_tree(g._h, ctypes.c_void_p(d.ptr), -1, None, 0, ctypes.byref(out)) == SBMP_ERR_INVALID_ARGUMENT
    assert L.sbmp_kgmt_recheck_tree(g._h, None, 5, None, 0, ctypes.byref(out)) == SBMP_ERR_INVALID_ARGUMENT
    assert L.sbmp_kgmt_recheck_tree(g._h, ctypes.c_void_p(d.ptr), 5, None, 0, ctypes.byref(out)) == 0   # NULL / 0: the summary
    R = out.rows
    assert R == min(g.result().treeSize, g.M) and out.alive == R
    small = np.zeros(R - 1, np.uint8)
    out2 = nat.TreeRecheck()
    assert L.sbmp_kgmt_recheck_tree(g._h, ctypes.c_void_p(d.ptr), 5, small.ctypes.data_as(ctypes.c_void_p), R - 1,
                                    ctypes.byref(out2)) == SBMP_ERR_INVALID_ARGUMENT
    assert out2.rows == R                                          # set in every case
    assert L.sbmp_kgmt_recheck_tree(g._h, None, 0, None, 0, ctypes.byref(out)) == 0 and out.alive == R   # an empty list
    g.query_goals([[1.0, 1.0]], 0.5, alive=True)
    g.step(3)
    assert g.result().treeSize > R
    assert status_of(lambda: g.query_goals([[1.0, 1.0]], 0.5, alive=True)) == SBMP_ERR_STATE   # the tree grew
    g.recheck(obstacles)
    g.query_goals([[1.0, 1.0]], 0.5, alive=True)
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    assert status_of(lambda: g.query_goals([[1.0, 1.0]], 0.5, alive=True)) == SBMP_ERR_STATE   # a new plan

"""GPU: k_tree_query and k_tree_query_alive (goal queries against tree rows, include/sbmp/tree_query.h).

Step level: sbmp_tree_query_batch on the crafted rows of tests/tree_query_cases.py against the
numpy model (tests/tree_query_model.py) and against the host twin, which applies the literal
sqrtf(d2) < r rule where the kernel compares d2 with a threshold; sbmp_tree_query_alive_batch
on the masked cases in the same way, against the model over the alive rows and the masked host
twin.  Planner level: KGMT.query_goals against the model over KGMT.tree(), after plan(), between
steps, on a local shard group and on a batch member, and KGMT.query_goals(alive=True) against
the step-level masked entry over the same tree.  Every comparison is bit-exact.

k_tree_query takes 2,048 rows per workgroup and step on a grid of at most 8 workgroups per CU:
one sweep is at most 4,194,304 rows on the 256 CUs of an MI355X, and the case single-4194381
goes round the grid-stride loop a second time.  k_tree_query_alive takes 256 rows per workgroup
and sweep on a grid of the same bound: one sweep is at most 524,288 rows, and masked-rows-524365
and masked-rows-1048577 hold alive inside rows, and the nearest row, in its second and third
sweep (with fewer resident workgroups the sweeps are shorter and those rows lie in later ones).
"""
import numpy as np
import pytest

from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, bits
from scenarios import BASE, BASE_SEED
from scenarios import random_boxes
from tree_query_cases import MASKED_NAMES, NAMES, case, check_expect, masked_case
from tree_query_model import FIELDS, assert_same_answers, model_of_rows, tree_rows
from tree_recheck_model import tree_arrays

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
SBMP_ERR_STATE = 5
WALL_GOAL = (9.0, 7.0)   # inside the (0,6)-(18,8) wall: a metre from any free point


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


def _model_of_tree(g, goals, radius=None):
    """The model over what tree() exports now, cut to the rows result() counts."""
    from cudasbmp_amd.tree_query import goal_array
    s, p, c = g.tree()
    state, ctrl = tree_rows(s, c, g.result().treeSize)
    return model_of_rows(state, ctrl, goal_array(goals, radius)), (s, p, c)


def _workspace_goals():
    """65 goals on a 13 x 5 grid over the 20 x 20 workspace, the demo goal, and one the tree
    cannot reach; all at r = 0.5."""
    gx, gy = np.meshgrid(np.linspace(0.75, 19.25, 13), np.linspace(1.0, 19.0, 5))
    g = np.stack([gx.ravel(), gy.ravel()], axis=1)
    return np.concatenate([g, [DEMO_GOAL[:2]], [WALL_GOAL]]).astype(np.float32)


# ---------------------------------------------------------------- step level
@pytest.mark.parametrize("name", NAMES)
def test_device_matches_model_and_host(name):
    from cudasbmp_amd import tree_query_batch
    state, ctrl, goals, expect, model = case(name)
    dev = tree_query_batch(state, ctrl, goals)
    assert_same_answers(dev, model, label=f"{name} device vs model")
    assert_same_answers(dev, tree_query_batch(state, ctrl, goals, device=False), label=f"{name} device vs host")
    check_expect(dev, expect, label=name)


@pytest.mark.parametrize("name", ["ties", "goals-65", "degenerate"])
def test_two_launches_give_identical_bytes(name):
    from cudasbmp_amd import tree_query_batch
    state, ctrl, goals = case(name)[:3]
    a, b = tree_query_batch(state, ctrl, goals), tree_query_batch(state, ctrl, goals)
    for k in FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_radius_argument_forms():
    from cudasbmp_amd import tree_query_batch
    state, ctrl, goals = case("goals-9")[:3]
    one = goals.copy()
    one[:, 2] = 1.25
    assert_same_answers(tree_query_batch(state, ctrl, one[:, :2], 1.25), tree_query_batch(state, ctrl, one))


# ---------------------------------------------------------------- step level, masked
@pytest.mark.parametrize("name", MASKED_NAMES)
def test_masked_device_matches_model_and_host(name):
    from cudasbmp_amd import tree_query_batch
    c = masked_case(name)   # where the mask must matter is asserted as the case is built
    dev = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask)
    assert_same_answers(dev, c.model, label=f"{name} device vs model")
    host = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask, device=False)
    assert_same_answers(dev, host, label=f"{name} device vs host")
    check_expect(dev, c.expect, label=name)


@pytest.mark.parametrize("name", ["masked-ties", "masked-goals-65", "masked-none"])
def test_two_masked_launches_give_identical_bytes(name):
    from cudasbmp_amd import tree_query_batch
    c = masked_case(name)
    a = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask)
    b = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask)
    for k in FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_any_nonzero_byte_is_alive():
    from cudasbmp_amd import tree_query_batch
    b, z = masked_case("masked-bytes"), masked_case("masked-bytes-01")
    assert np.array_equal(b.mask != 0, z.mask == 1) and ((b.mask & 1) == 0).sum() > 1000
    got = tree_query_batch(b.state, b.ctrl, b.goals, alive=b.mask)
    assert_same_answers(got, tree_query_batch(z.state, z.ctrl, z.goals, alive=z.mask), label="bytes vs 0 / 1")
    assert_same_answers(got, z.model, label="bytes vs the 0 / 1 model")


@pytest.mark.parametrize("name", ["ties", "radius-edges", "degenerate", "overflow", "random"])
def test_a_mask_of_ones_gives_the_unmasked_answers(name):
    from cudasbmp_amd import tree_query_batch
    state, ctrl, goals, expect, model = case(name)
    unmasked = tree_query_batch(state, ctrl, goals)
    for byte in (1, 0xff):
        got = tree_query_batch(state, ctrl, goals, alive=np.full(len(state), byte, np.uint8))
        assert_same_answers(got, unmasked, label=f"{name} masked kernel vs unmasked kernel")
        assert_same_answers(got, model, label=f"{name} masked kernel vs model")
        check_expect(got, expect, label=name)


# ---------------------------------------------------------------- planner level
def test_planner_masked_query_equals_the_step_level_entry(obstacles):
    """After recheck(), query_goals(alive=True) is sbmp_tree_query_alive_batch over tree() and the
    mask status == 0 (FREE and not CUT: alive)."""
    from cudasbmp_amd import tree_query_batch
    g = _mk(**BASE)
    g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=BASE_SEED)
    other = random_boxes(600, 20.0, 20.0, 7, 0.3, 0.8)
    status, summary = g.recheck(other)
    s, p, c = g.tree()
    state, ctrl, parent = tree_arrays(s, p, c, g.result().treeSize)
    alive = status == 0
    assert len(alive) == len(state) and 1 < summary["alive"] == alive.sum() < len(alive)
    goals = np.concatenate([_workspace_goals(), np.full((67, 1), 0.5, np.float32)], axis=1)
    got = g.query_goals(goals, alive=True)
    assert_same_answers(got, tree_query_batch(state, ctrl, goals, alive=alive), label="planner vs step level")
    assert_same_answers(got, model_of_rows(state, ctrl, goals, alive), label="planner vs model")
    assert (got["count"] > 0).any() and (got["count"] == 0).any()
    assert got["count"].tobytes() != g.query_goals(goals)["count"].tobytes()   # the mask matters


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_query_of_the_plans_own_goal(seed, obstacles):
    g = _mk()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0
    a = g.query_goals([DEMO_GOAL[:2]], DEMO["goalThreshold"])
    s, p, c = g.tree()
    assert a["firstRow"][0] == r.goalIndex
    assert a["count"][0] >= 1
    best = int(a["bestRow"][0])
    assert bits(a["bestCost"])[0] == bits(c[best:best + 1])[0]
    assert a["bestCost"][0] <= np.float32(g.costToGoal_)
    rows, ps, pc = g.solution_path(best)
    assert rows[0] == 0 and rows[-1] == best and bits(pc[-1:])[0] == bits(a["bestCost"])[0]
    assert_same_answers(a, _model_of_tree(g, [DEMO_GOAL[:2]], DEMO["goalThreshold"])[0], label=f"seed {seed}")


@pytest.mark.parametrize("fix", [False, True])
def test_every_field_over_a_full_tree(fix, obstacles):
    """goalThreshold = 0: the plan runs until the tree is full.  Under the reference's partial
    clear (fix = False, D6) counted rows may never have been written: the query reads what
    tree() shows."""
    g = _mk(goalThreshold=0.0, fixGNewClear=fix)
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=1)
    assert r.goalIndex == -1
    goals = _workspace_goals()
    a = g.query_goals(goals, 0.5)
    model, _ = _model_of_tree(g, goals, 0.5)
    assert_same_answers(a, model, label=f"full tree fix={fix}")
    assert a["count"][-2] >= 1       # the demo goal's disc holds rows
    assert a["nearestRow"][-1] >= 0 and a["nearestDistance"][-1] > 0
    if fix:   # every row was a valid child: none lies inside a box
        assert a["count"][-1] == 0 and a["firstRow"][-1] == -1 and a["nearestDistance"][-1] >= 0.5
    three = np.concatenate([goals, np.full((len(goals), 1), 0.5, np.float32)], axis=1)
    assert_same_answers(g.query_goals(three), a, label="(Q, 3) form")


def test_query_between_steps_changes_nothing(obstacles):
    kw = dict(BASE)
    goals = _workspace_goals()

    def run(query):
        g = _mk(**kw)
        g.begin(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), BASE_SEED)
        seen = []
        for _ in range(2):
            g.step(3)
            if query:
                a = g.query_goals(goals, 0.5)
                model, _ = _model_of_tree(g, goals, 0.5)
                assert_same_answers(a, model, label=f"after {3 * (len(seen) + 1)} iterations")
                seen.append(a)
        while g.step(4):
            pass
        return g, seen

    g0, _ = run(False)
    g1, seen = run(True)
    assert seen[0]["count"].tobytes() != seen[1]["count"].tobytes()   # the tree grew between the two queries
    assert g1.state_hash() == g0.state_hash()
    for x, y in zip(g1.tree(), g0.tree()):
        assert np.array_equal(bits(x), bits(y))
    r0, r1 = g0.result(), g1.result()
    assert (r1.iterations, r1.treeSize, r1.accepted) == (r0.iterations, r0.treeSize, r0.accepted)
    assert_same_answers(g1.query_goals(goals, 0.5), g0.query_goals(goals, 0.5), label="at the end")


def test_local_group_and_batch_member_answer_as_one_planner(obstacles):
    from cudasbmp_amd import KGMTBatch
    kw = dict(BASE)
    goals = _workspace_goals()
    d = _dev(obstacles)
    single = _mk(**kw)
    single.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    want = single.query_goals(goals, 0.5)
    assert_same_answers(want, _model_of_tree(single, goals, 0.5)[0], label="single")
    group = _mk(_local_group=2, **kw)
    group.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    assert_same_answers(group.query_goals(goals, 0.5), want, label="local group of 2")
    cfg, extra = _split(kw)
    b = KGMTBatch(2, **cfg, **extra)
    b.plan([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d, len(obstacles), [BASE_SEED + 1, BASE_SEED])
    assert_same_answers(b[1].query_goals(goals, 0.5), want, label="batch member 1")
    assert_same_answers(b[0].query_goals(goals, 0.5), _model_of_tree(b[0], goals, 0.5)[0], label="batch member 0")


def test_query_before_begin_is_a_state_error():
    from cudasbmp_amd import SbmpError
    g = _mk()
    with pytest.raises(SbmpError) as e:
        g.query_goals([DEMO_GOAL[:2]], 0.5)
    assert e.value.status == SBMP_ERR_STATE
    with pytest.raises(SbmpError) as e:
        g.query_goals([[np.nan, 1.0]], 0.5)
    assert e.value.status == 1   # SBMP_ERR_INVALID_ARGUMENT: the arguments are checked first

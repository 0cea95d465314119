"""GPU parity over family I (tests/goal_scenarios.py): the goal verdict at equality and one
ulp either side, and which row ends the plan, in every form that restates the decision --
k_step's accept-time test with its lane / wave / block-word / scan reductions and the
jGoal < nIns && jGoal < M - tsPrev clamp, the sharded k_step's row scan and rank-word walk
(groups of 2 and 3), the two-launch form's insert_block (one insert workgroup per block, at
16,384 slots), insert_blocks (262,400 slots = 1,025 blocks, the smallest shape at which
k_finish groups blocks) and insert_records (a group of 2 under SBMP_STEP=0), k_step_batch
per member, sbmp_insert_batch's k_insert, and the three host plan loops.

Every planner run asserts
  - the whole state against the oracle, bit for bit (assert_same_state);
  - goalIndex, iterations, treeSize and the bits of costToGoal against the float32 numpy
    model on pass 0, which shares no goal code with the oracle;
  - solution_path() against pass 0's parent chain, ending on the model's row;
and the triples that `at` and `out` agree and differ from `in` in the expected way.  No
tolerances: every comparison is exact.

tests/test_goal_scenarios_oracle.py shows (without a GPU) that each case reaches its edge.
"""
import numpy as np
import pytest

from conftest import bits
from goal_scenarios import (BIG, CAPACITY_IDS, GROUPED, INSERT_IDS, KINDS, NOWHERE, S16, THRESHOLD_IDS, VARIANTS,
                            capacity_cases, discs, insert_cases, insert_inputs, model, pass0, scenario, threshold_cases,
                            verdict)
from test_goal_scenarios_oracle import check_insert, oracle_run
from test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu

F32 = np.float32
# name -> (environment, local shard group, the form path_info must report)
FORMS = {
    "k_step": ({}, 0, "k_step"),
    "two-launch": ({"SBMP_STEP": "0"}, 0, "two-launch"),                    # insert_block
    "group2": ({}, 2, "k_step"),
    "group3": ({}, 3, "k_step"),
    "group2-two-launch": ({"SBMP_STEP": "0"}, 2, "two-launch"),             # insert_records
    "two-launch-grouped": ({}, 0, "two-launch"),                            # insert_blocks: 1,025 blocks
}
SMALL_FORMS = ("k_step", "two-launch", "group2", "group3", "group2-two-launch")
VERDICT_PARAMS = [(f, S16, it) for f in SMALL_FORMS for it in (1, 3)] + [("two-launch-grouped", GROUPED, 1)]
DISC_PARAMS = ([(f, S16, n) for f in SMALL_FORMS for n in KINDS[S16]] + [("k_step", BIG, n) for n in KINDS[BIG]]
               + [("two-launch-grouped", GROUPED, n) for n in KINDS[GROUPED]])


def planner(form, sc, monkeypatch, count=0):
    from cudasbmp_amd import KGMT, KGMTBatch
    env, group, _ = FORMS[form]
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    return KGMTBatch(count, **cfg, **extra) if count else KGMT(**cfg, **extra, _local_group=group)


def device_boxes(sc):
    from cudasbmp_amd import DeviceBuffer
    obs = sc.obstacles()
    return (DeviceBuffer(obs) if len(obs) else None), len(obs)


def check(g, form, shape, goal, thr, limit=None):
    """A finished planner (or batch member) against the oracle and against the model on pass 0."""
    _, group, step_form = FORMS[form]
    info = g.path_info()
    assert info["form"] == step_form and info["nranks"] == max(1, group), info
    assert_same_state(g, oracle_run(shape, goal, thr, limit), check_unexplored=True, label=f"{form} {shape}")
    p, e, r = pass0(shape), model(shape, goal, thr, limit), g.result()
    got = (r.goalIndex, r.iterations, r.treeSize, int(F32(r.costToGoal).view(np.uint32)))
    assert got == (e.goalIndex, e.iterations, e.treeSize, e.cost_bits), f"planner {got}, model {e}"
    rows, samples, costs = g.solution_path()
    assert tuple(rows.tolist()) == e.path
    assert np.array_equal(bits(samples), bits(p.samples[rows])) and np.array_equal(bits(costs), bits(p.costs[rows]))
    return e


def run(form, shape, goal, thr, monkeypatch, limit=None):
    sc = scenario(shape, goal, thr, limit)
    g = planner(form, sc, monkeypatch)
    d_obs, n = device_boxes(sc)
    g.plan(sc.initial7(), sc.goal7(), d_obs, n, seed=sc.seed)
    return check(g, form, shape, goal, thr, limit)


@pytest.mark.parametrize("form,shape,it", VERDICT_PARAMS, ids=[f"{f}-{s}-verdict-it{it}" for f, s, it in VERDICT_PARAMS])
def test_verdict_triple(form, shape, it, oracle_lib, monkeypatch):
    v = verdict(shape, it)
    e_at, e_in, e_out = (run(form, shape, v.goal, v.thr(k), monkeypatch) for k in VARIANTS)
    assert (e_in.goalIndex, e_in.iterations) == (v.row, it)
    assert e_at == e_out and e_at.goalIndex != v.row


@pytest.mark.parametrize("form,shape,name", DISC_PARAMS, ids=[f"{f}-{s}-lowest-{n}" for f, s, n in DISC_PARAMS])
def test_lowest_row_wins(form, shape, name, oracle_lib, monkeypatch):
    d = discs(shape)[name]
    e = run(form, shape, d.goal, d.thr, monkeypatch)
    assert (e.goalIndex, e.iterations) == (d.rows[0], 1)


@pytest.mark.parametrize("k", range(len(CAPACITY_IDS)), ids=[f"k_step-capacity-{n}" for n in CAPACITY_IDS])
def test_capacity(k, oracle_lib, monkeypatch):
    c = capacity_cases()[k]
    e = run("k_step", c.shape, c.goal, c.thr, monkeypatch)
    if c.row is not None:
        assert e.goalIndex == c.row


@pytest.mark.parametrize("form", ("k_step", "two-launch", "group2"))
@pytest.mark.parametrize("it", (1, 3))
def test_iteration_limit(it, form, oracle_lib, monkeypatch):
    v = verdict(S16, it)
    last = run(form, S16, v.goal, v.thr("in"), monkeypatch, limit=it)      # the flush pass inserts the row
    assert (last.goalIndex, last.iterations) == (v.row, it)
    short = run(form, S16, v.goal, v.thr("in"), monkeypatch, limit=it - 1)
    assert (short.goalIndex, short.iterations) == (-1, it - 1)


@pytest.mark.parametrize("k", range(len(THRESHOLD_IDS)), ids=[f"k_step-threshold-{n}" for n in THRESHOLD_IDS])
def test_threshold(k, oracle_lib, monkeypatch):
    _, goal, thr = threshold_cases()[k]
    run("k_step", S16, goal, thr, monkeypatch)


def test_batch_members(oracle_lib, monkeypatch):
    """One KGMTBatch carries the 16k shape's discs, a goal each under the shared radius, and one
    member whose goal is never reached: k_step_batch runs the body per member."""
    ds = list(discs(S16).values())
    goals = [d.goal for d in ds] + [NOWHERE]
    thr = S16.radius
    sc = scenario(S16, NOWHERE, thr)
    b = planner("k_step", sc, monkeypatch, count=len(goals))
    d_obs, n = device_boxes(sc)
    res = b.plan([sc.initial7()] * len(goals), [tuple(g) + (0.0,) * 5 for g in goals], d_obs, n, [sc.seed] * len(goals))
    info = b.info()
    assert info["batched"] == 1 and info["launchesPerIteration"] == 1, info
    for i, goal in enumerate(goals):
        e = check(b[i], "k_step", S16, goal, thr)
        assert (res[i].goalIndex, res[i].iterations) == (e.goalIndex, e.iterations)
    assert [r.goalIndex for r in res] == [d.rows[0] for d in ds] + [-1]
    assert res[-1].iterations == S16.passes


@pytest.mark.parametrize("k", range(len(INSERT_IDS)), ids=INSERT_IDS)
def test_insert_batch_on_the_device(k, oracle_lib):
    from cudasbmp_amd.batch import insert_batch
    from oracle.pyoracle import insert_batch as oracle_insert
    _, shape, goal, thr = insert_cases()[k]
    fix = bool(dict(fixGNewClear=True, **shape.kw)["fixGNewClear"])
    args = insert_inputs(shape)
    got = insert_batch(*args, goal, thr, fix)
    check_insert(shape, goal, thr, got)
    want = oracle_insert(*args, goal, thr, fix)
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(bits(a), bits(b))
    assert got[4:] == want[4:]


def test_plan_loops(oracle_lib, monkeypatch):
    """plan() (the polled loop), begin() + step(1) until it returns false, and begin() + enqueue(n)
    far past the goal's iteration + sync(): launches queued behind a found goal are no-ops."""
    v = verdict(S16, 3)
    goal, thr, limit = v.goal, v.thr("in"), 12
    sc = scenario(S16, goal, thr, limit)
    d_obs, n = device_boxes(sc)
    seen = []
    for how in ("plan", "step", "enqueue"):
        g = planner("k_step", sc, monkeypatch)
        if how == "plan":
            g.plan(sc.initial7(), sc.goal7(), d_obs, n, seed=sc.seed)
        else:
            g.begin(sc.initial7(), sc.goal7(), d_obs, n, sc.seed)
            if how == "step":
                steps = 1
                while g.step(1):
                    steps += 1
                assert steps == v.it
            else:
                g.enqueue(limit - 2)
                g.sync()
        e = check(g, "k_step", S16, goal, thr, limit)
        assert (e.goalIndex, e.iterations) == (v.row, v.it)
        r = g.result()
        seen.append((r.iterations, r.treeSize, r.goalIndex, int(F32(r.costToGoal).view(np.uint32)), r.samplesGenerated,
                     r.accepted, r.stalled, g.state_hash()))
    assert seen[0] == seen[1] == seen[2], seen

"""GPU: KGMTBatch (several independent queries, one k_step_batch launch per iteration)
against the CPU oracle, member by member.

Every comparison is the whole state of a member against its own oracle run
(tests/test_gpu_parity.assert_same_state): tree, parents, costs, G / GNew, the region
arrays, the unexplored slots, RNG, iteration log and result, bit for bit.  An oracle run
is computed once per (configuration, boxes, root, goal, seed) and only read afterwards.
"""
import ctypes

import numpy as np
import pytest

from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL
from scenarios import BASE, random_boxes
from test_gpu_parity import _oracle, assert_same_state

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
# distinct roots near the demo's (clear of its boxes), and the demo goal
ROOTS = [DEMO_INITIAL, (5.5, 4.5, 0.3, 0.0, 0, 0, 0), (4.5, 5.25, -1.0, 0.5, 0, 0, 0), (3.0, 3.0, 2.0, 0.0, 0, 0, 0),
         (6.0, 4.0, 1.0, 1.0, 0, 0, 0)]

_ORACLES = {}


def _split(kw):
    cfg = dict(DEMO)
    kw = dict(kw)
    extra = {k: kw.pop(k) for k in EXTRA_KEYS if k in kw}
    cfg.update(kw)
    return cfg, extra


def _mkb(count, **kw):
    from cudasbmp_amd import KGMTBatch
    cfg, extra = _split(kw)
    return KGMTBatch(count, **cfg, **extra), cfg, extra


def _mk1(**kw):
    from cudasbmp_amd import KGMT
    cfg, extra = _split(kw)
    return KGMT(**cfg, **extra)


def _planned_oracle(cfg, extra, obs, init, goal, seed):
    key = (tuple(sorted(cfg.items())), tuple(sorted(extra.items())), obs.tobytes(), tuple(init), tuple(goal), seed)
    if key not in _ORACLES:
        o = _oracle(cfg, extra, threads=16)
        o.plan(init, goal, obs, seed)
        _ORACLES[key] = o
    return _ORACLES[key]


def _dev(obs):
    from cudasbmp_amd import DeviceBuffer
    return DeviceBuffer(obs) if len(obs) else None


def _check_members(b, cfg, extra, obs, inits, goals, seeds, label=""):
    for i in range(len(b)):
        o = _planned_oracle(cfg, extra, obs, inits[i], goals[i], seeds[i])
        assert_same_state(b[i], o, label=f"{label} member {i} seed {seeds[i]}")


def _plan_and_check(B, kw, obs, seeds=None, inits=None, goals=None, label=""):
    b, cfg, extra = _mkb(B, **kw)
    seeds = list(seeds if seeds is not None else range(11, 11 + B))
    inits = list(inits if inits is not None else [ROOTS[i % len(ROOTS)] for i in range(B)])
    goals = list(goals if goals is not None else [DEMO_GOAL] * B)
    res = b.plan(inits, goals, _dev(obs), len(obs), seeds)
    assert len(res) == B
    _check_members(b, cfg, extra, obs, inits, goals, seeds, label=label)
    for i, r in enumerate(res):   # plan()'s results are the members' own
        q = b.result(i)
        assert (r.iterations, r.treeSize, r.goalIndex, r.accepted) == (q.iterations, q.treeSize, q.goalIndex, q.accepted)
        assert r.wallMs > 0.0
    return b, res


def test_demo_one_launch(obstacles, oracle_lib):
    seeds = (1, 2, 3, 7)
    b, res = _plan_and_check(4, {}, obstacles, seeds=seeds, inits=[DEMO_INITIAL] * 4, label="demo")
    info = b.info()
    assert info["batched"] == 1 and info["launchesPerIteration"] == 1 and info["membersPerLaunch"] == 4
    assert info["count"] == 4 and info["groupsPerMember"] == 119
    assert info["residentGroups"] >= 4 * 119
    d = _dev(obstacles)
    for i, seed in enumerate(seeds):
        g = _mk1()
        r = g.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=seed)
        assert r.goalIndex == res[i].goalIndex and r.iterations == res[i].iterations
        for x, y in zip(g.solution_path(), b[i].solution_path()):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert b[i].path_info()["form"] == "k_step"


def test_members_ending_at_different_iterations(obstacles, oracle_lib):
    inits = [DEMO_INITIAL] * 3
    goals = [DEMO_GOAL,
             (6.0, 5.0, 0, 0, 0, 0, 0),    # one metre from the root
             (9.0, 7.0, 0, 0, 0, 0, 0)]    # inside the (0,6)-(18,8) wall: more than the radius from any free point
    seeds = [1, 2, 3]
    b, res = _plan_and_check(3, {}, obstacles, seeds=seeds, inits=inits, goals=goals, label="ends")
    its = [r.iterations for r in res]
    assert len(set(its)) == 3, its
    assert res[0].goalIndex >= 0 and res[1].goalIndex >= 0 and res[2].goalIndex == -1
    assert its[1] < its[0] < its[2]
    assert res[2].treeSize >= DEMO["maxTreeSize"] or its[2] == DEMO["numIterations"]
    assert res[1].wallMs <= res[2].wallMs
    d = _dev(obstacles)
    for i in (0, 1):   # what they held at their own end, however long the batch ran on
        g = _mk1()
        g.plan(inits[i], goals[i], d, len(obstacles), seed=seeds[i])
        assert b[i].state_hash() == g.state_hash(), f"member {i}"


def test_split_by_residency(obstacles, oracle_lib, monkeypatch):
    monkeypatch.setenv("SBMP_BATCH_MAX_GROUPS", str(2 * 119 + 7))   # two demo members fit
    b, _ = _plan_and_check(5, {}, obstacles, label="cap")
    info = b.info()
    assert info["residentGroups"] == 2 * 119 + 7
    assert info["launchesPerIteration"] == 3 and info["membersPerLaunch"] == 2 and info["batched"] == 1
    monkeypatch.setenv("SBMP_BATCH_MAX_GROUPS", "1000000")   # never raises the device's figure
    one, _ = _plan_and_check(1, {}, obstacles, label="one")
    i1 = one.info()
    assert i1["batched"] == 1 and i1["launchesPerIteration"] == 1
    assert 119 <= i1["residentGroups"] < 1000000
    monkeypatch.delenv("SBMP_BATCH_MAX_GROUPS")
    B = i1["residentGroups"] // i1["groupsPerMember"] + 1
    b, _ = _plan_and_check(B, {}, obstacles, seeds=[1 + (i % 4) for i in range(B)],
                           inits=[ROOTS[(i // 4) % len(ROOTS)] for i in range(B)], label="device")
    info = b.info()
    assert info["residentGroups"] == i1["residentGroups"]
    assert info["launchesPerIteration"] == 2 and info["membersPerLaunch"] == B - 1


def test_member_that_does_not_fit_runs_two_launches(obstacles, oracle_lib, monkeypatch):
    monkeypatch.setenv("SBMP_BATCH_MAX_GROUPS", "100")   # below one demo member's 119
    b, _ = _plan_and_check(2, {}, obstacles, label="no fit")
    info = b.info()
    assert info["batched"] == 0 and info["launchesPerIteration"] == 2
    assert b[0].path_info()["form"] == "two-launch"


SMALL = {
    "one-block": dict(maxTreeSize=256),                                      # 2 workgroups per member; k = 0 iterations
    "k<32": dict(maxTreeSize=5000, samplesPerIteration=1000),                # k < 32, and a tree that fills
    "fill-n1": dict(batchRule="fill", samplesPerIteration=4096, fixGNewClear=True, goalThreshold=0.0,
                    numIterations=40, maxTreeSize=200000, n=1),
    "fill-n8": dict(batchRule="fill", samplesPerIteration=4096, fixGNewClear=True, goalThreshold=0.0,
                    numIterations=40, maxTreeSize=200000, n=8),
    "fill-n16": dict(batchRule="fill", samplesPerIteration=4096, fixGNewClear=True, goalThreshold=0.0,
                     numIterations=40, maxTreeSize=200000, n=16),            # direct R2 atomics (no key log)
    # kFoldEvery is 64: here the key-log fold runs inside the batch's loop
    "fill-n8-fold": dict(batchRule="fill", samplesPerIteration=2048, fixGNewClear=True, goalThreshold=0.0,
                         numIterations=70, maxTreeSize=160000, n=8),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_smallest_shapes(name, obstacles, oracle_lib):
    b, res = _plan_and_check(3, SMALL[name], obstacles, label=name)
    assert b.info()["batched"] == 1
    logs = [b[i].iter_log() for i in range(3)]
    if name == "one-block":   # 256 rows: k falls to 0 after two iterations and the loop idles to numIterations
        assert b.info()["groupsPerMember"] == 2
        assert all((l[:, 3] == 0).any() for l in logs)
    if name == "k<32":        # the capacity rule gives k < 32 from the third iteration on; the tree fills
        assert all((l[2:, 3] < 32).all() for l in logs)
        assert all(r.treeSize >= 5000 and r.iterations < DEMO["numIterations"] for r in res)
    if name == "fill-n8-fold":
        assert all(r.iterations == 70 for r in res)


def _boxes(kind, obstacles):
    if kind == "none":
        return np.zeros((0, 4), dtype=np.float32)
    if kind == "nine":
        more = np.array([[10, 12, 11, 13], [14, 3, 15, 4], [12, 15, 13, 16], [16, 10, 17, 11]], dtype=np.float32)
        return np.concatenate([obstacles, more])
    if kind == "600":
        return random_boxes(600, 20.0, 20.0, seed=7, hmax=0.3, clear=1.2)
    if kind == "3000":
        return random_boxes(3000, 20.0, 20.0, seed=8, hmax=0.08, clear=1.2)
    return obstacles


# (name, planner kwargs over BASE, boxes, SBMP_EXPAND_VARIANT, SBMP_STEP, expected obstacle form)
FORMS = [
    ("point", dict(agent="point"), "demo", None, None, "registers"),
    ("numDisc13", dict(numDisc=13), "demo", None, None, "registers"),
    ("length1.3", dict(agentLength=1.3), "demo", None, None, "registers"),
    ("no-boxes", dict(), "none", None, None, "registers"),
    ("nine-lds", dict(), "nine", None, None, "lds"),
    ("600-lds", dict(), "600", None, None, "lds"),
    ("600-grid", dict(), "600", "4", None, "grid"),
    ("3000-grid", dict(), "3000", None, None, "grid"),
    ("3000-global", dict(), "3000", "5", None, "global"),
    ("two-launch", dict(), "demo", None, "0", "registers"),
]


@pytest.mark.parametrize("name,kw,boxes,variant,step,form", FORMS, ids=[f[0] for f in FORMS])
def test_forms(name, kw, boxes, variant, step, form, obstacles, oracle_lib, monkeypatch):
    if variant is not None:
        monkeypatch.setenv("SBMP_EXPAND_VARIANT", variant)
    if step is not None:
        monkeypatch.setenv("SBMP_STEP", step)
    obs = _boxes(boxes, obstacles)
    full = dict(BASE)   # 16,384 slots, 12 iterations, as the scenario matrix
    full.update(kw)
    b, res = _plan_and_check(3, full, obs, label=name)
    info = b.info()
    for i in range(3):
        pi = b[i].path_info()
        assert pi["obstacle_form"] == form, pi
        assert pi["form"] == ("two-launch" if step == "0" else "k_step")
    if step == "0":
        assert info["batched"] == 0 and info["launchesPerIteration"] == 3
    else:
        assert info["batched"] == 1 and info["launchesPerIteration"] == 1 and info["groupsPerMember"] == 65
    assert all(r.iterations == 12 for r in res)


def test_stepwise(obstacles, oracle_lib):
    b, cfg, extra = _mkb(3)
    seeds = [42, 43, 44]
    inits = ROOTS[:3]
    goals = [DEMO_GOAL] * 3
    os_ = [_oracle(cfg, extra) for _ in range(3)]
    b.begin(inits, goals, _dev(obstacles), len(obstacles), seeds)
    for i in range(3):
        os_[i].begin(inits[i], goals[i], obstacles, seeds[i])
    for it in range(1, 6):
        running = b.step(1)
        for i in range(3):
            assert os_[i].step()
            assert_same_state(b[i], os_[i], label=f"iteration {it} member {i}")
        assert running == 3, "no demo query ends within five iterations"
    assert b.info()["batched"] == 1
    # enqueue / sync: three more iterations without waiting in between
    b.enqueue(3)
    b.sync()
    for i in range(3):
        for _ in range(3):
            os_[i].step()
        assert_same_state(b[i], os_[i], label=f"enqueue member {i}")


def test_reuse_identity_and_permutation(obstacles, oracle_lib):
    d = _dev(obstacles)
    b, cfg, extra = _mkb(3)
    goals = [DEMO_GOAL] * 3
    b.plan(ROOTS[:3], goals, d, len(obstacles), [1, 2, 3])
    first = [b[i].state_hash() for i in range(3)]
    # a second plan on the same batch, other seeds and roots
    inits2, seeds2 = [ROOTS[3], ROOTS[4], ROOTS[1]], [21, 22, 23]
    b.plan(inits2, goals, d, len(obstacles), seeds2)
    _check_members(b, cfg, extra, obstacles, inits2, goals, seeds2, label="second plan")
    second = [b[i].state_hash() for i in range(3)]
    assert second != first
    for i in range(3):
        g = _mk1()
        g.plan(inits2[i], goals[i], d, len(obstacles), seed=seeds2[i])
        assert g.state_hash() == second[i], f"member {i} differs from a fresh single plan"
    # permuting the members permutes the results and changes nothing else
    perm = [2, 0, 1]
    p, _, _ = _mkb(3)
    rp = p.plan([inits2[j] for j in perm], goals, d, len(obstacles), [seeds2[j] for j in perm])
    assert [p[i].state_hash() for i in range(3)] == [second[j] for j in perm]
    assert [r.iterations for r in rp] == [b.result(j).iterations for j in perm]
    # a batch of one is KGMT.plan
    one, cfg1, extra1 = _mkb(1)
    r1 = one.plan([DEMO_INITIAL], [DEMO_GOAL], d, len(obstacles), [7])[0]
    g = _mk1()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=7)
    assert (r1.iterations, r1.treeSize, r1.goalIndex) == (r.iterations, r.treeSize, r.goalIndex)
    assert one[0].state_hash() == g.state_hash()
    _check_members(one, cfg1, extra1, obstacles, [DEMO_INITIAL], [DEMO_GOAL], [7], label="B=1")


def test_profiled_batch_launches(obstacles):
    b, _, _ = _mkb(2, profileKernels=True)
    res = b.plan(ROOTS[:2], [DEMO_GOAL] * 2, _dev(obstacles), len(obstacles), [1, 2])
    launches, ms = b.kernel_stats()["k_step_batch"]
    assert launches >= max(r.iterations for r in res) and ms > 0.0
    assert b[0].kernel_stats()["k_step"][0] == 0   # no member launched k_step itself


def test_wait_error_names_a_member(obstacles, monkeypatch):
    from cudasbmp_amd._native import SbmpError
    monkeypatch.setenv("SBMP_INJECT_WAIT_ERROR", "1")
    b, _, _ = _mkb(3, numIterations=2000, maxTreeSize=1 << 18, goalThreshold=0.0)
    d = _dev(obstacles)
    with pytest.raises(SbmpError) as e:
        b.plan(ROOTS[:3], [DEMO_GOAL] * 3, d, len(obstacles), [1, 2, 3])
    assert "member 0" in str(e.value) and "hand-off" in str(e.value)
    ran = len(b[0].iter_log())   # the injected error stops the host loop, not the kernels
    assert 0 < ran <= 8, ran
    monkeypatch.delenv("SBMP_INJECT_WAIT_ERROR")
    res = b.plan(ROOTS[:3], [DEMO_GOAL] * 3, d, len(obstacles), [1, 2, 3])   # the next plan starts clean
    assert all(r.iterations > 8 for r in res)


def test_argument_errors(obstacles):
    from cudasbmp_amd import KGMTBatch
    from cudasbmp_amd import _native as nat
    d = _dev(obstacles)
    with pytest.raises(nat.SbmpError) as e:
        KGMTBatch(0, **DEMO)
    assert e.value.status == 1
    b, _, _ = _mkb(2)
    bad = [DEMO_INITIAL, (5.0, float("nan"), 0, 0, 0, 0, 0)]
    with pytest.raises(nat.SbmpError) as e:   # D15, before anything is launched
        b.plan(bad, [DEMO_GOAL] * 2, d, len(obstacles), [1, 2])
    assert e.value.status == 1 and "member 1" in str(e.value)
    i = np.zeros((2, 7), dtype=np.float32)
    s = np.zeros(2, dtype=np.uint64)
    vp = ctypes.c_void_p
    for args in ((None, i.ctypes.data_as(vp), s.ctypes.data_as(vp)), (i.ctypes.data_as(vp), None, s.ctypes.data_as(vp)),
                 (i.ctypes.data_as(vp), i.ctypes.data_as(vp), None)):
        st = nat.lib().sbmp_kgmt_batch_begin(b._h, args[0], args[1], vp(d.ptr), len(obstacles), args[2])
        assert st == 1
    with pytest.raises(nat.SbmpError) as e:
        b.step(1)   # no begin() yet
    assert e.value.status == 5


def test_borrowed_member_is_read_only(obstacles):
    from cudasbmp_amd import _native as nat
    d = _dev(obstacles)
    b, _, _ = _mkb(2)
    b.plan(ROOTS[:2], [DEMO_GOAL] * 2, d, len(obstacles), [1, 2])
    m = b[0]
    for call in (lambda: m.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=1),
                 lambda: m.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), 1),
                 lambda: m.step(1), lambda: m.enqueue(1),
                 lambda: nat.call("sbmp_kgmt_destroy", m._h)):
        with pytest.raises(nat.SbmpError) as e:
            call()
        assert e.value.status == 5   # SBMP_ERR_STATE
    with pytest.raises(nat.SbmpError) as e:
        m.set_iteration_dump("/tmp/never-written")
    assert e.value.status == 6   # SBMP_ERR_UNSUPPORTED
    assert m.result().iterations == b.result(0).iterations   # reads still work
    with pytest.raises(nat.SbmpError):
        b.result(2)

"""GPU: a used planner handle plans bit for bit like a fresh one (tests/reuse_scenarios.py).

Each sequence runs on ONE handle.  After every plan of it (not only the last):
  1. the whole state -- iteration log, tree rows, G / GNew, the eight region tables, the
     unexplored slots, RNG states, the result -- equals a fresh CPU oracle run of that plan
     alone (tests/test_gpu_parity.assert_same_state); every plan that is begun and then driven
     by hand (stepped, enqueued, abandoned) is compared in the same way right after begin()
     too, with an oracle that has only begun;
  2. path_info() names the step form and obstacle form the table names for that plan, so the
     transition really happened;
  3. state_hash() equals that of a fresh handle of the same configuration that ran only that
     plan: a second witness over the replicated state, and the only one that sees the ctrl
     blocks.
tests/test_reuse_scenarios_oracle.py shows (without a GPU) that each predecessor leaves
behind what its successor is sensitive to.
"""
import ctypes

import numpy as np
import pytest

import reuse_scenarios as rs
from reuse_scenarios import BATCH_IDS, BATCHES, IDS, SEQUENCES, oracle_begun, oracle_run
from test_gpu_parity import assert_same_state
from tree_recheck_model import assert_same_recheck, recheck_model, tree_arrays

pytestmark = pytest.mark.gpu

ENV_KEYS = ("SBMP_STEP", "SBMP_EXPAND_VARIANT")
QUERY_GOALS = np.array([[2.0, 18.0], [10.0, 10.0], [6.5, 5.0]], dtype=np.float32)
_FRESH = {}


def _dev(obs):
    from cudasbmp_amd import DeviceBuffer
    return DeviceBuffer(obs) if len(obs) else None


def _handle(seq):
    from cudasbmp_amd import KGMT
    cfg, extra = seq.config()
    return KGMT(**cfg, **extra, _local_group=seq.local_group)


def _clobber(d):
    """The caller reuses its obstacle array for another map, then frees it."""
    from cudasbmp_amd import _native as nat
    other = np.ascontiguousarray(rs.grid_3000()[:5], dtype=np.float32)
    assert other.size == d.count
    nat.call("sbmp_device_copy_to", ctypes.c_void_p(d.ptr), other.ctypes.data_as(ctypes.c_void_p), other.nbytes)
    d.free()


def _drive(g, plan, hooks=(), begun=None):
    """Run `plan` on handle g the way the table says; the hooks, and begun() (the state right
    after begin()), between begin() and the first step."""
    from cudasbmp_amd._native import SbmpError
    obs = plan.obstacles()
    d = _dev(obs)
    if plan.drive == "plan":
        assert not {"alive_raises", "clobber"} & set(hooks), "these run between begin() and the first step"
        g.plan(plan.initial7(), plan.goal7(), d, len(obs), seed=plan.seed)
        return
    g.begin(plan.initial7(), plan.goal7(), d, len(obs), plan.seed)
    if "alive_raises" in hooks:   # the last re-check's alive mask was of another tree
        with pytest.raises(SbmpError) as e:
            g.query_goals(QUERY_GOALS, radius=0.5, alive=True)
        assert e.value.status == 5, e.value   # SBMP_ERR_STATE
    if "clobber" in hooks:
        _clobber(d)
    if begun is not None:
        begun()
    if plan.drive == "step":
        while g.step(7):
            pass
    elif plan.drive == "enqueue":
        g.enqueue(plan.iterations)          # not waited for: the next begin() meets it in flight
    elif plan.drive == "abandon":
        g.step(plan.iterations)
        g.tree()
    else:
        raise AssertionError(plan.drive)


def _fresh_hash(seq, plan):
    """state_hash() of a fresh handle of seq's configuration that ran only `plan`."""
    cfg, extra = seq.config()
    key = (tuple(sorted(cfg.items())), tuple(sorted(extra.items())), tuple(sorted(seq.env.items())), seq.local_group,
           plan.obstacles().tobytes(), plan.initial, plan.goal, plan.seed, plan.drive == "abandon" and plan.iterations)
    if key not in _FRESH:
        g = _handle(seq)
        _drive(g, plan if plan.drive == "abandon" else rs._with(plan, drive="plan", hooks=()))
        _FRESH[key] = g.state_hash()
        g.close()
    return _FRESH[key]


def _tree_passes(g):
    """The grown-tree passes, whose scratch, alive mask and obstacle staging the next begin() meets."""
    r = g.result()
    rows = min(r.treeSize, g.M)
    status, summary = g.recheck(rs.lds_600())
    assert summary["rows"] == rows == len(status)
    answers = g.query_goals(QUERY_GOALS, radius=0.5, alive=True)
    assert len(answers["count"]) == len(QUERY_GOALS)
    steps, st = g.trace()
    assert steps.shape == (rows, g.numDisc_, 4) and len(st) == rows
    paths = g.solution_paths([r.goalIndex, rows - 1, -1])
    assert paths["status"].tolist() == [0, 0, 1] and paths["lengths"][0] > 1


def _recheck_equals_model(g, seq, label):
    cfg, extra = seq.config()
    boxes = rs.lds_600()
    s, p, c = g.tree()
    state, ctrl, parent = tree_arrays(s, p, c, g.result().treeSize)
    want, wsum, _ = recheck_model(state, ctrl, parent, boxes, numDisc=cfg["numDisc"], agentLength=cfg["agentLength"],
                                  width=cfg["width"], height=cfg["height"], agent=extra.get("agent", "car"))
    assert wsum["rows"] == len(state)
    assert_same_recheck(g.recheck(boxes), (want, wsum), label=label)


@pytest.mark.parametrize("seq", SEQUENCES, ids=IDS)
def test_sequence_on_one_handle(seq, oracle_lib, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in seq.env.items():
        monkeypatch.setenv(k, v)
    big = seq.config()[0]["maxTreeSize"] > rs.CACHE_ROWS
    g = _handle(seq)
    for i, plan in enumerate(seq.plans):
        label = f"{seq.name} plan {i} ({plan.tag})"
        # right after begin(): the constructor state, whatever the last plan left (R1Score 1.0
        # in the buffer of even iterations, which iteration 1 never writes, is seen only here)
        _drive(g, plan, hooks=plan.hooks, begun=lambda: assert_same_state(
            g, oracle_begun(seq, plan), check_unexplored=True, label=label + " after begin()"))
        info = g.path_info()
        assert info["form"] == seq.step_form(i), f"{label}: {info}"
        assert info["obstacle_form"] == plan.obstacle_form, f"{label}: {info}"
        assert info["nranks"] == max(1, seq.local_group), f"{label}: {info}"
        if plan.drive == "enqueue":
            continue   # in flight: the next begin() is the next thing this handle sees
        o = oracle_run(seq, plan, threads=16 if big else 8)
        assert_same_state(g, o, check_unexplored=True, label=label)
        del o
        assert g.state_hash() == _fresh_hash(seq, plan), f"{label}: digest differs from a fresh handle's"
        if "passes" in plan.hooks:
            _tree_passes(g)
        if "recheck" in plan.hooks:
            _recheck_equals_model(g, seq, label)
    g.close()


@pytest.mark.parametrize("bs", BATCHES, ids=BATCH_IDS)
def test_batch_sequence_on_one_batch(bs, oracle_lib, monkeypatch):
    """S12: consecutive plan() calls of one KGMTBatch with other boxes, roots and seeds; the
    number of launches a batch is packed into depends on the obstacle form."""
    from conftest import DEMO
    from cudasbmp_amd import KGMTBatch
    for k in ENV_KEYS + ("SBMP_BATCH_MAX_GROUPS",):
        monkeypatch.delenv(k, raising=False)
    seq = bs.member_sequence()
    b = KGMTBatch(bs.count, **DEMO)
    launches = []
    for row in bs.plans:
        tag, boxes, form, roots, goals, seeds = row
        obs = np.ascontiguousarray(boxes(), dtype=np.float32).reshape(-1, 4)
        plans = [bs.member_plan(row, i) for i in range(bs.count)]
        res = b.plan([p.initial7() for p in plans], [p.goal7() for p in plans], _dev(obs), len(obs), list(seeds))
        assert len(res) == bs.count
        info = b.info()
        assert info["batched"] == 1, f"{bs.name} {tag}: {info}"
        launches.append(info["launchesPerIteration"])
        for i, p in enumerate(plans):
            label = f"{bs.name} {tag} member {i}"
            pi = b[i].path_info()
            assert pi["form"] == "k_step" and pi["obstacle_form"] == form, f"{label}: {pi}"
            assert_same_state(b[i], oracle_run(seq, p), check_unexplored=True, label=label)
            assert b[i].state_hash() == _fresh_hash(seq, p), f"{label}: digest differs from a fresh single handle's"
    if bs.count >= 12:
        assert max(launches) > 1, f"{bs.name}: launches per iteration {launches}"
    b.close()

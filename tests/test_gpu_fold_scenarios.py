"""GPU parity over family K (tests/fold_scenarios.py): the fold of the R2 key log inside runs that
pass its 64-iteration window with a varying S, so that a ring row still holds, at and past S(t),
the keys of iteration t - 64 (or of an earlier plan on the same handle), in every form that
drives the fold:

  k_step / two-launch   plan(): the automatic fold every 64 iterations and the one at the export
  stepwise              exports in mid-window: step(30) and the state at 30 (the pending window
                        folded early, the next automatic fold takes rows 31 .. 63, then 0 .. 30),
                        step(64) and the state at 94, step(1) and the state at 95, then the rest
  stepwise-fold         the same with fold() + sync() in place of the first export
  enqueue               enqueue(140) + sync()
  group2 / group3       local shard groups: the rank term of the slot
  batch                 a KGMTBatch of three members under different seeds
  used handle           100 iterations under another seed, then the scenario: the handle's ring
                        holds the earlier plan's keys

Each form is asserted through path_info and compares the whole state with the oracle, bit for
bit (assert_same_state: the eight region tables among it).  tests/test_fold_scenarios_oracle.py
shows (without a GPU) that every scenario reaches the stale part of the ring.
"""
import pytest

import fold_scenarios as fs
from conftest import DEMO_GOAL, DEMO_INITIAL
from fold_scenarios import ITERATIONS, oracle_at
from test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu

# name -> (environment, local shard group, the form path_info must report)
FORMS = {
    "k_step": ({}, 0, "k_step"),
    "two-launch": ({"SBMP_STEP": "0"}, 0, "two-launch"),
    "group2": ({}, 2, "k_step"),
    "group3": ({}, 3, "k_step"),
}
OTHER_SEED = 5


def planner(form, sc, monkeypatch, count=0):
    from cudasbmp_amd import KGMT, KGMTBatch
    env, group, _ = FORMS[form]
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    return KGMTBatch(count, **cfg, **extra) if count else KGMT(**cfg, **extra, _local_group=group)


@pytest.fixture(scope="module")
def boxes(oracle_lib):
    from cudasbmp_amd import DeviceBuffer, fold_r2_info
    assert fold_r2_info(256)["window"] == fs.WINDOW
    obs = fs.obstacles()
    return DeviceBuffer(obs), len(obs)


def check_path(g, form):
    _, group, step_form = FORMS[form]
    info = g.path_info()
    assert info["form"] == step_form and info["nranks"] == max(1, group), info


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", fs.IDS)
def test_plan(name, form, boxes, monkeypatch):
    sc = fs.BY_NAME[name]
    g = planner(form, sc, monkeypatch)
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, boxes[0], boxes[1], seed=sc.seed)
    check_path(g, form)
    assert r.iterations >= 2 * fs.WINDOW
    assert_same_state(g, oracle_at(name), label=f"{form} {name}")


@pytest.mark.parametrize("first", ["export", "fold"])
@pytest.mark.parametrize("form", ["k_step", "two-launch"])
@pytest.mark.parametrize("name", fs.IDS)
def test_stepwise_exports_in_mid_window(name, form, first, boxes, monkeypatch):
    sc = fs.BY_NAME[name]
    g = planner(form, sc, monkeypatch)
    g.begin(DEMO_INITIAL, DEMO_GOAL, boxes[0], boxes[1], sc.seed)
    check_path(g, form)
    assert g.step(30)
    if first == "export":
        assert_same_state(g, oracle_at(name, 30), label=f"{form} {name} at 30")
    else:
        g.fold()
        g.sync()
    assert g.step(fs.WINDOW)
    assert_same_state(g, oracle_at(name, 30 + fs.WINDOW), label=f"{form} {name} at 94")
    assert g.step(1)
    assert_same_state(g, oracle_at(name, 31 + fs.WINDOW), label=f"{form} {name} at 95")
    g.step(ITERATIONS)
    assert_same_state(g, oracle_at(name), label=f"{form} {name} at the end")


@pytest.mark.parametrize("form", ["k_step", "two-launch"])
@pytest.mark.parametrize("name", fs.IDS)
def test_enqueue_all_then_sync(name, form, boxes, monkeypatch):
    sc = fs.BY_NAME[name]
    g = planner(form, sc, monkeypatch)
    g.begin(DEMO_INITIAL, DEMO_GOAL, boxes[0], boxes[1], sc.seed)
    check_path(g, form)
    g.enqueue(ITERATIONS)
    g.sync()
    assert_same_state(g, oracle_at(name), label=f"{form} {name} enqueued")


@pytest.mark.parametrize("name", fs.IDS)
def test_batch_of_three_seeds(name, boxes, monkeypatch):
    sc = fs.BY_NAME[name]
    seeds = [sc.seed, sc.seed + 1, OTHER_SEED]
    b = planner("k_step", sc, monkeypatch, count=3)
    b.plan([DEMO_INITIAL] * 3, [DEMO_GOAL] * 3, boxes[0], boxes[1], seeds)
    info = b.info()
    assert info["batched"] == 1, info
    for i, seed in enumerate(seeds):
        check_path(b[i], "k_step")
        assert_same_state(b[i], oracle_at(name, None, seed), label=f"batch member {i} {name}")


@pytest.mark.parametrize("form", ["k_step", "two-launch"])
@pytest.mark.parametrize("name", fs.IDS)
def test_used_handle_folds_like_a_fresh_one(name, form, boxes, monkeypatch):
    sc = fs.BY_NAME[name]
    g = planner(form, sc, monkeypatch)
    g.begin(DEMO_INITIAL, DEMO_GOAL, boxes[0], boxes[1], OTHER_SEED)
    assert g.step(100)
    assert_same_state(g, oracle_at(name, 100, OTHER_SEED), label=f"{form} {name} earlier plan")
    g.plan(DEMO_INITIAL, DEMO_GOAL, boxes[0], boxes[1], seed=sc.seed)
    check_path(g, form)
    assert_same_state(g, oracle_at(name), label=f"{form} {name} on a used handle")
    fresh = planner(form, sc, monkeypatch)
    fresh.plan(DEMO_INITIAL, DEMO_GOAL, boxes[0], boxes[1], seed=sc.seed)
    assert g.state_hash() == fresh.state_hash()

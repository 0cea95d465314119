"""The HIP kernels against the reference's own text, with no oracle in between:
oracle/_ref/libkgmt_ref.so holds the reference's propagateAndCheck, getR1 and getR2, compiled
unmodified for the host (see tests/test_reference_text.py and tests/reference_text.py), and the
kernels' children, verdicts, RNG states and region counters are held to those functions' results.

  - sbmp_expand_batch on the device: children, valid and RNG states against propagateAndCheck,
    r1 / r2 (getR1_k / getR2_k) against getR1 / getR2, at widths 20 and 17.3;
  - the planner's own kernels: after begin(), rng(), step(1), unexplored(), tree(), iter_log() and
    regions() are read, and every slot the iteration expanded is replayed through the reference's
    functions (reference_text.check_step), for each obstacle form of family H at its equality
    variants (registers, lds, lds x 4, the grid behind k_step's LDS table and k_expand's global one,
    the global loop, the NaN filler), the two-launch form, a shard group of 2, a KGMTBatch's members,
    and three scenarios of tests/scenarios.py (the Payne-Hanek heading, L = 2, width 17.3).

These tests read the built library alone, never the reference tree; a missing library is an error,
not a skip.  Each case is 16,384 slots and 3 iterations.
"""
import numpy as np
import pytest

import reference_text as rt
from conftest import bits
from edge_scenarios import FORMS, box_case, pass0, wall_case
from scenarios import SCENARIOS
from test_batch import _obstacle_sets
from test_reference_text import K, batch, check_cells

pytestmark = pytest.mark.gpu

ITERATIONS = 3


@pytest.fixture(scope="module")
def ref(oracle_lib):
    return rt.lib()


# ---------------------------------------------------------------- sbmp_expand_batch on the device
@pytest.mark.parametrize("obs_name", ["demo", "c5"])
@pytest.mark.parametrize("numDisc,L,width", [(10, 1.0, 20.0), (7, 1.3, 17.3)])
def test_expand_batch_on_the_device(obs_name, numDisc, L, width, obstacles, ref):
    """4,096 parents fill several workgroups; without the last one the tail is ragged."""
    from cudasbmp_amd.batch import expand_batch
    obs = _obstacle_sets(obstacles)[obs_name]
    parents, states = batch(K, 11 + numDisc, width, 20.0)
    r = ref.ref_expand(parents, states, obs, numDisc, L, width, 20.0)
    assert 0.02 <= r["valid"].mean() <= 0.98
    for k in (K, K - 1):
        g = expand_batch(parents[:k], states[:k], obs, numDisc=numDisc, agentLength=L, width=width, device=True)
        assert np.array_equal(bits(g["children"]), bits(r["children"][:k]))
        assert np.array_equal(g["valid"].astype(bool), r["valid"][:k])
        assert np.array_equal(g["rng"], r["rng"][:k])
        xy = np.ascontiguousarray(r["children"][:k, :2])
        r1, _, ok = check_cells(ref, xy, width, 8, others=(("the device", (g["r1"], g["r2"])),))
        assert ok.all() and (r1 >= 0).any() and (r1 < 0).any()


# ---------------------------------------------------------------- the planner's own kernels
def make_planner(sc, monkeypatch, count=0):
    from cudasbmp_amd import KGMT, DeviceBuffer, KGMTBatch
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    obs = sc.obstacles()
    d_obs = DeviceBuffer(obs) if len(obs) else None
    if count:
        g = KGMTBatch(count, **cfg, **extra)
        g.begin([sc.initial7()] * count, [sc.goal7()] * count, d_obs, len(obs), [sc.seed + i for i in range(count)])
        members = [g[i] for i in range(count)]
    else:
        g = KGMT(**cfg, **extra, _local_group=sc.local_group)
        g.begin(sc.initial7(), sc.goal7(), d_obs, len(obs), sc.seed)
        members = [g]
    for m in members:
        info = m.path_info()
        assert info["form"] == sc.step_form, info
        assert info["obstacle_form"] == sc.obstacle_form, info
        assert info["nranks"] == max(1, sc.local_group), info
    return g, members


def replay_planner(sc, monkeypatch, label):
    g, _ = make_planner(sc, monkeypatch)
    r = rt.replay(g, sc, iterations=ITERATIONS, label=label)
    print(f"{label}: {r.iterations} iterations, {r.slots} slots, valid share {r.share:.4f}")
    assert r.iterations == ITERATIONS and 0.02 <= r.share <= 0.98
    return r


def edge_case(form, group, variant="at"):
    return (box_case if group == "box" else wall_case)(form, variant)


def check_chosen(form, group, first):
    """At equality the reference's <= leaves the chosen children free of the slab, and its >= puts
    the chosen pair outside the wall."""
    p0 = pass0(form)
    chosen = p0.chosen if group == "box" else sorted({p0.extremes["+x"], p0.extremes["+y"]})
    assert (first.valid[chosen] == (group == "box")).all(), first.valid[chosen]


EDGE_FORMS = ("H1-fast-sched-E", "H6-lds", "H6-lds4", "H7-grid-lds-table", "H8-grid-global-table", "H9-global",
              "H10-grid-nan", "H11-two-launch", "H12-group2")
EDGE_PARAMS = [(f, g) for f in FORMS if f.name in EDGE_FORMS for g in ("box", "wall")]
assert len(EDGE_PARAMS) == 2 * len(EDGE_FORMS)


@pytest.mark.parametrize("form,group", EDGE_PARAMS, ids=[f"{f.name}-{g}" for f, g in EDGE_PARAMS])
def test_planner_on_verdict_edges(form, group, ref, monkeypatch):
    sc = edge_case(form, group)
    r = replay_planner(sc, monkeypatch, f"{form.name}-{group}-at")
    check_chosen(form, group, r.first)


SCENARIO_NAMES = ("B-theta+105610", "C-L2", "A-17.3x20-car-registers")


@pytest.mark.parametrize("name", SCENARIO_NAMES)
def test_planner_on_scenarios(name, ref, monkeypatch):
    sc = next(s for s in SCENARIOS if s.name == name)
    replay_planner(sc, monkeypatch, name)


@pytest.mark.parametrize("group", ["box", "wall"])
def test_batch_members(group, ref, monkeypatch):
    """Two members of one KGMTBatch (k_step_batch), the case's own query and the same root under
    another seed, each replayed on every iteration."""
    form = next(f for f in FORMS if f.name == "H1-fast-sched-E")
    sc = edge_case(form, group)
    b, members = make_planner(sc, monkeypatch, count=2)
    info = b.info()
    assert info["batched"] == 1 and info["launchesPerIteration"] == 1, info
    slots, valid = [0, 0], [0, 0]
    for it in range(ITERATIONS):
        befores = [rt.before(m) for m in members]
        b.step(1)
        for i, m in enumerate(members):
            st = rt.check_step(m, sc, befores[i], True, label=f"batch member {i} {form.name}-{group} iteration {it + 1}")
            assert st is not None
            slots[i] += st.S
            valid[i] += int(st.valid.sum())
            if i == 0 and it == 0:
                check_chosen(form, group, st)
    for i in range(2):      # over the whole replay, as for a single planner
        print(f"batch member {i}: {slots[i]} slots, valid share {valid[i] / slots[i]:.4f}")
        assert 0.02 <= valid[i] / slots[i] <= 0.98

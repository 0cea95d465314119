"""GPU parity over family J (tests/region_scenarios.py): which R1 / R2 cell a child falls in,
what the region counters and R1Score become and whether the child is accepted, at the edges
of each decision, in every form that restates them -- k_step's bins_k (the reciprocal
division and the IEEE one, asserted through path_info's rcp_divisions), k_expand of the
two-launch form (SBMP_STEP=0), a shard group of 2 (the counter deltas cross the exchange),
k_step_batch per member, sbmp_expand_batch's kernel with the public headers' getR1 / getR2,
and the host's binning of the root at begin().

Every planner is stepped one iteration at a time and asserts, after each step,
  - the region counters, R1Score, the inserted rows (the accept bits in slot order) and the
    RNG states against the float32 numpy model, which shares no code with the oracle or the
    kernels; no tolerance and no excused child;
and at its end
  - the whole state against the oracle, bit for bit (assert_same_state), and the model's
    accept bits of every iteration against those it gave for the oracle.

tests/test_region_scenarios_oracle.py shows (without a GPU) that each case reaches its edge.
"""
import numpy as np
import pytest

from region_scenarios import CASE_IDS, branch, cases, check_trace, root_case, scenario, sizes, snapshot, trace
from test_gpu_parity import assert_same_state
from test_region_scenarios_oracle import (EXPAND_NAMES, accept_at_equality, check_expand_case, check_root, oracle_run,
                                          seen_of)

pytestmark = pytest.mark.gpu

# name -> (environment, local shard group, the form path_info must report)
FORMS = {
    "k_step": ({}, 0, "k_step"),
    "two-launch": ({"SBMP_STEP": "0"}, 0, "two-launch"),
    "group2": ({}, 2, "k_step"),
}
# a shard group of 2: the round-up triples' first members, the R2 gap and the concentration
GROUP_NAMES = [k for k in CASE_IDS if k.endswith(("-up", "-on")) or k.startswith(("J-gap", "J-conc"))]
PARAMS = [(name, form) for name in CASE_IDS for form in ("k_step", "two-launch")] + [(n, "group2") for n in GROUP_NAMES]
# one batch per parameter set: the first member of each planted kind, on both division branches
BATCH_NAMES = ["J-r1-x-odd-small-up", "J-r1-y-odd-small-up", "J-r1-y-odd-large-up", "J-r1-y-pow2-large-on", "J-minus1-x-in", "J-fma-n3-small", "J-fma-n8-large",
               "J-gap-n11-small", "J-gap-n12-large"]


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


def check_path(g, form, c):
    """The step form, the group size and the division branch the case claims, as begin() chose them."""
    from cudasbmp_amd.kgmt import division_reciprocal
    _, group, step_form = FORMS[form]
    info = g.path_info()
    assert info["form"] == step_form and info["nranks"] == max(1, group), info
    R1Size, R2Size = sizes(c.width, c.n)
    rcp = info["rcp_divisions"]
    assert rcp["R1Size"] == (division_reciprocal(float(R1Size)) != 0.0), info
    assert rcp["R2Size"] == (division_reciprocal(float(R2Size)) != 0.0), info
    assert rcp["numDisc"] and rcp["agentLength"], info
    took = "rcp" if rcp["R1Size"] and rcp["R2Size"] else "ieee"
    assert took == branch(c.width, c.n) == ("ieee" if c.site == "large" else "rcp")


def check_end(g, name, seen, label):
    o, _ = oracle_run(name)
    assert_same_state(g, o, check_unexplored=True, label=label)
    want = seen_of(name)
    assert len(seen) == len(want)
    for a, b in zip(seen, want):
        assert a.S == b.S and np.array_equal(a.accept, b.accept)
        assert np.array_equal(a.r1, b.r1) and np.array_equal(a.r2, b.r2)


@pytest.mark.parametrize("name,form", PARAMS, ids=[f"{f}-{n}" for n, f in PARAMS])
def test_case(name, form, oracle_lib, monkeypatch):
    c = cases()[name]
    sc = scenario(c)
    g = planner(form, sc, monkeypatch)
    d_obs, n = device_boxes(sc)
    g.begin(sc.initial7(), sc.goal7(), d_obs, n, sc.seed)
    check_path(g, form, c)
    seen = check_trace(c, trace(c, g), label=f"{form} {name}")
    check_end(g, name, seen, f"{form} {name}")


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_batch_members(name, oracle_lib, monkeypatch):
    """Two members on the case's parameter set, the case's own query and the same root under another
    seed: k_step_batch runs the body per member, and the model holds for each on every iteration."""
    c = cases()[name]
    sc = scenario(c)
    b = planner("k_step", sc, monkeypatch, count=2)
    d_obs, n = device_boxes(sc)
    b.begin([sc.initial7()] * 2, [sc.goal7()] * 2, d_obs, n, [sc.seed, sc.seed + 1])
    info = b.info()
    assert info["batched"] == 1 and info["launchesPerIteration"] == 1, info
    snaps = [[snapshot(b[i])] for i in range(2)]
    for _ in range(c.iterations):
        b.step(1)
        for i in range(2):
            snaps[i].append(snapshot(b[i]))
    for i in range(2):
        check_path(b[i], "k_step", c)
        seen = check_trace(c, snaps[i], label=f"batch member {i} {name}")
        assert len(seen) == c.iterations
        if i == 0:
            check_end(b[0], name, seen, f"batch member 0 {name}")


@pytest.mark.parametrize("name", EXPAND_NAMES)
def test_expand_batch_on_the_device(name, oracle_lib):
    check_expand_case(name, device=True)


def test_accept_at_equality_on_the_device(oracle_lib):
    accept_at_equality(device=True)


@pytest.mark.parametrize("form", ("k_step", "two-launch", "group2"))
def test_root_binning(form, oracle_lib, monkeypatch):
    """The host bins the root at begin() (getR1 / getR2 of the public headers, IEEE): a root the float
    division rounds up onto a cell line lands in that cell's sub-column 0."""
    c = root_case()
    sc = scenario(c)
    g = planner(form, sc, monkeypatch)
    g.begin(sc.initial7(), sc.goal7(), None, 0, sc.seed)
    check_root(c, g.regions())
    check_trace(c, trace(c, g), label=f"{form} root")

"""GPU parity over family H (tests/edge_scenarios.py): box edges and walls on a child's own
float, and one ulp either side, in every form that restates the reference's predicates --
the fast car loop with and without the schedule, L = 2, car_euler under wave_cull,
point_euler, the LDS lists, the grid behind k_step's LDS table and k_expand's global one,
the global loop, the batched form under obsNaN, the two-launch form, a shard group of 2,
their one-step twins, and the public headers behind sbmp_expand_batch.

Every (form, case group) runs its three variants, one planner run each, and asserts
  - the whole state against the oracle, bit for bit, after three iterations;
  - without the oracle: between the variants the planner's own valid and invalid counts of
    iteration 1 move by the expected flips (box: `in` turns the chosen children invalid,
    `out` equals `at`; mid: `in` stops the one chosen child), and the children that were
    valid in pass 0 are stored as in pass 0 (the wall group of the multi-step forms has no
    such count check -- R1Size moves with width -- and rests on the oracle comparison alone);
  - for the one-step forms: the planner's counts equal the reference's comparisons in numpy
    (collisionCheck.cu:6-28) applied to the planner's own child array, walls included;
  - sbmp_expand_batch on the device: the same box and wall cases, `valid` compared directly.

tests/test_edge_scenarios_oracle.py shows (without a GPU) that each case reaches its edge.
"""
import numpy as np
import pytest

from conftest import bits
from edge_scenarios import (GROUP_IDS, GROUP_PARAMS, GROUPS, SLOTS, VARIANTS, in_r1_grid, mid_probe, pass0,
                            reference_invalid)
from scenarios import make_oracle
from test_edge_scenarios_oracle import HEADER_FORMS, check_header_batch, header_batch
from test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu


def run(form, sc, monkeypatch):
    """One planner run of `sc`: (children, valid count, invalid count) of iteration 1, then the
    final state against the oracle."""
    from cudasbmp_amd import KGMT, DeviceBuffer
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    obs = sc.obstacles()
    g = KGMT(**cfg, **extra, _local_group=sc.local_group)
    d_obs = DeviceBuffer(obs)
    g.begin(sc.initial7(), sc.goal7(), d_obs, len(obs), sc.seed)
    info = g.path_info()
    assert info["form"] == sc.step_form, info
    assert info["obstacle_form"] == sc.obstacle_form, info
    assert info["nranks"] == max(1, sc.local_group), info
    g.step(1)
    u = g.unexplored()[0][:SLOTS].copy()
    reg = g.regions()
    counts = int(reg["R1Valid"].sum()), int(reg["R1Invalid"].sum())
    g.step(cfg["numIterations"] - 1)
    assert_same_state(g, make_oracle(sc), check_unexplored=True, label=sc.name)
    if form.one_step:
        invalid = reference_invalid(form.root, u, obs, cfg["width"], cfg["height"])
        grid = in_r1_grid(u, cfg["width"])
        assert counts == (int((~invalid & grid).sum()) + 1, int((invalid & grid).sum())), "the numpy predicate"
    return u, counts


@pytest.mark.parametrize("form,group", GROUP_PARAMS, ids=GROUP_IDS)
def test_verdict_edges(form, group, oracle_lib, monkeypatch):
    p0 = pass0(form)
    res = {v: run(form, GROUPS[group](form, v), monkeypatch) for v in VARIANTS}
    (u_at, n_at), (u_in, n_in), (u_out, n_out) = (res[v] for v in VARIANTS)
    if group == "box":
        k = form.flips
        assert n_out == n_at and n_in == (n_at[0] - k, n_at[1] + k), f"at {n_at}, in {n_in}, out {n_out}"
        keep = p0.valid | form.one_step
        for u in (u_at, u_in, u_out):
            assert (bits(u[keep]) == bits(p0.children[keep])).all()
    elif group == "mid":
        slot, xs = mid_probe(form)
        assert n_out == n_at and np.array_equal(bits(u_at), bits(u_out))
        changed = np.nonzero((bits(u_at) != bits(u_in)).any(axis=1))[0]
        assert changed.tolist() == [slot] and u_in[slot, 0] == xs
        assert n_in[0] + n_in[1] == n_at[0] + n_at[1] and n_in[1] >= n_at[1]
    else:   # walls: R1Size moves with width, so the oracle is the judge; the chosen pair keeps its (x, y)
        pair = sorted({p0.extremes["+x"], p0.extremes["+y"]})
        for u in (u_at, u_in, u_out):
            assert (bits(u[pair, :2]) == bits(p0.children[pair, :2])).all()


@pytest.mark.parametrize("form", HEADER_FORMS, ids=[f.name for f in HEADER_FORMS])
def test_public_headers_on_the_device(form, oracle_lib):
    check_header_batch(form, *header_batch(form, device=True))

"""GPU parity over the scenario table (tests/scenarios.py): the HIP planner against the
CPU oracle, bit for bit, at the edges of the hot loop's shortcuts -- non-square
workspaces, root headings at the sine / cosine reduction limits, power-of-two
wheelbases other than 1, moving roots, the schedule's size limit, degenerate boxes --
in the one-launch form, the two-launch form and local shard groups.

tests/test_scenarios_oracle.py shows (without a GPU) that each scenario reaches its edge.
"""
import pytest

from scenarios import IDS, SCENARIOS, make_oracle
from test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_scenario_bit_exact(sc, oracle_lib, monkeypatch):
    from cudasbmp_amd import KGMT, DeviceBuffer
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    obs = sc.obstacles()
    g = KGMT(**cfg, **extra, _local_group=sc.local_group)
    d_obs = DeviceBuffer(obs) if len(obs) else None
    g.plan(sc.initial7(), sc.goal7(), d_obs, len(obs), seed=sc.seed)
    info = g.path_info()
    assert info["form"] == sc.step_form, info
    assert info["obstacle_form"] == sc.obstacle_form, info
    assert info["nranks"] == max(1, sc.local_group), info
    o = make_oracle(sc)
    assert_same_state(g, o, check_unexplored=True, label=sc.name)

"""The HIP planner held to the independent float64 model of tests/f64_model.py: the same
audit_run that tests/test_f64_audit_oracle.py applies to the CPU oracle, on
cudasbmp_amd.KGMT stepped one iteration at a time, one scenario per form of the hot
loop (register / LDS / grid boxes, car and point, the two wheelbase forms, a moving root,
a corner root, both sides of the schedule's size limit, NaN and infinite boxes, the
two-launch form, a shard group, and a Payne-Hanek heading with the loose cap); then
sbmp_expand_batch's device kernel child by child, and the goal row of the demo.

No oracle here: the kernels are compared with the model alone, so a misreading of the
reference that kernels and oracle share cannot pass.  The planner is bit-exact with the
oracle (tests/test_gpu_scenarios.py), so the figures are those of
tests/test_f64_audit_oracle.py's docstring: worst err / bound ratio 0.996 over the
scenarios below (0.996 on F-nan-low), borderline + edge share 0.001 % .. 0.15 % (B-theta+3e5:
27.8 %), each scenario as in that docstring's table; the run on an MI355X measured the same.
"""
import numpy as np
import pytest

import f64_model as model
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL
from scenarios import SCENARIOS
from test_f64_audit_oracle import BATCH_CASES, audit_expand_batch, audit_scenario

pytestmark = pytest.mark.gpu

# name -> iterations (None: 12, or 4 from 600 boxes on, as on the oracle)
GPU_AUDITED = {
    "base": None,
    "A-30x12-car-registers": None,
    "A-12x30-car-lds": 4,
    "A-17.3x20-car-grid": 4,
    "A-30x12-point-registers": None,
    "C-L2": None,
    "C-L0.5": None,
    "D-v-25": None,
    "D-corner": None,
    "E-7boxes-8steps": None,
    "E-0boxes-65steps": None,
    "F-nan-low": None,
    "F-inf-wall": None,
    "G-C-L2-two-launch": None,
    "G-A-30x12-car-registers-group2": None,
    "B-theta+3e5": None,      # the loose cap (test_f64_audit_oracle.LOOSE)
}
BY_NAME = {s.name: s for s in SCENARIOS}


@pytest.mark.parametrize("name", list(GPU_AUDITED))
def test_planner_against_f64_model(name, monkeypatch):
    from cudasbmp_amd import KGMT, DeviceBuffer
    sc = BY_NAME[name]
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    obs = sc.obstacles()
    g = KGMT(**cfg, **extra, _local_group=sc.local_group)
    d_obs = DeviceBuffer(obs) if len(obs) else None
    g.begin(sc.initial7(), sc.goal7(), d_obs, len(obs), sc.seed)
    info = g.path_info()
    assert info["form"] == sc.step_form and info["obstacle_form"] == sc.obstacle_form, info
    assert info["nranks"] == max(1, sc.local_group), info
    st = audit_scenario(g, sc, iters=GPU_AUDITED[name])
    print(name, {k: (round(v, 6) if isinstance(v, float) else v) for k, v in st.items()})
    assert st["children"] >= 16384 and st["state_rows"] > 0 and st["accepted"] > 0 and st["iterations"] >= 3


@pytest.mark.parametrize("agent,obs_name,numDisc,L", BATCH_CASES)
def test_expand_batch_device_against_f64_model(agent, obs_name, numDisc, L, obstacles):
    audit_expand_batch(agent, obs_name, numDisc, L, obstacles, device=True)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_demo_goal_row(seed, obstacles):
    from cudasbmp_amd import KGMT, DeviceBuffer
    g = KGMT(**DEMO)
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, DeviceBuffer(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0, "demo seeds 1-3 solve"
    chain = model.audit_goal(g.tree(), g.iter_log(), r.goalIndex, r.costToGoal, DEMO_GOAL, DEMO["goalThreshold"])
    rows, samples, costs = g.solution_path()
    assert rows.tolist() == chain and rows[0] == 0
    s, _, c = g.tree()
    assert np.array_equal(samples.view(np.uint32), s[rows].view(np.uint32))
    assert np.array_equal(costs.view(np.uint32), c[rows].view(np.uint32))

"""GPU: the device forms of the uniform-grid obstacle index against brute force, at the segments
of tests/grid_cases.py (tests/test_grid_cases_oracle.py proves on the CPU what they cover).

Polylines.  sbmp_tree_recheck_batch replays every polyline case (point agent, numDisc = 1: row
r - 1 -> row r is one segment) under SBMP_EXPAND_VARIANT
    4   the grid behind the global cell-start table, B = 4 (grid_run / grid_run_sep); the batched
        reference form (grid_motion_valid_batched) for the lists with a NaN box
    0   automatic: the grid for the lists of 16,000 boxes, registers or the LDS list below
    5   the global all-boxes loop (the LDS list up to 2,048 boxes)
    2   the LDS-4 form, for the lists that fit it
and the status bytes and the summary equal the model's (the oracle's all-boxes replay), which
tests/test_grid_cases_oracle.py holds to the brute force and to the numpy walk.  Each case runs
twice in one process and gives the same bytes.

Planner scenarios.  k_step's B = 8 walk over the LDS cell-start table takes only the planner's own
draws: the scenarios of grid_cases.SCENARIOS (16,000 boxes under the clamp G = 90, clusters of 9, 17
and 33 boxes beside the root, a fast car) run against the CPU oracle with the full-state comparison
of tests/test_gpu_scenarios.py, in k_step, the two-launch form and local shard groups.

No case is built to make a kernel fault: the queries in and across the last cell are ordinary
queries with a known answer.
"""
import pytest

import grid_cases as gc
from scenarios import make_oracle
from test_gpu_parity import assert_same_state
from tree_recheck_model import assert_same_recheck

pytestmark = pytest.mark.gpu

MAX_LDS_BOXES = 2048            # kMaxLdsObs: longer lists take the grid (or the global loop under variant 5)
BOXES = {"g90": 16000, "g90-30x12": 16000}
POLY_FORMS = [(name, build, v) for name, build in gc.POLYLINES for v in ("4", "0", "5", "2")
              if v != "2" or BOXES.get(name, 0) <= MAX_LDS_BOXES]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


@pytest.mark.parametrize("name, build, variant", POLY_FORMS, ids=[f"{n}-variant{v}" for n, _, v in POLY_FORMS])
def test_polyline_bytes_equal_the_model(name, build, variant, monkeypatch):
    from cudasbmp_amd import tree_recheck_batch
    monkeypatch.setenv("SBMP_EXPAND_VARIANT", variant)
    c = build()
    case = c.case
    assert (len(case.boxes) <= MAX_LDS_BOXES) == (BOXES.get(name, 0) <= MAX_LDS_BOXES)
    status, summary, _ = case.model
    first = tree_recheck_batch(case.state, case.ctrl, case.parent, case.boxes, **case.params)
    again = tree_recheck_batch(case.state, case.ctrl, case.parent, case.boxes, **case.params)
    print(f"{name} variant {variant}: rows {len(status)} boxes {len(case.boxes)} G {c.g} summary {first[1]}")
    assert_same_recheck(first, (status, summary), label=f"{name} variant {variant} device vs model")
    assert first[0].tobytes() == again[0].tobytes() and first[1] == again[1]


@pytest.mark.parametrize("sc", gc.SCENARIOS, ids=gc.SCENARIO_IDS)
def test_scenario_bit_exact(sc, monkeypatch):
    from cudasbmp_amd import KGMT, DeviceBuffer
    for k in ("SBMP_STEP", "SBMP_EXPAND_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    cfg, extra = sc.config()
    obs = sc.obstacles()
    g = KGMT(**cfg, **extra, _local_group=sc.local_group)
    g.plan(sc.initial7(), sc.goal7(), DeviceBuffer(obs), len(obs), seed=sc.seed)
    info = g.path_info()
    print(f"{sc.name}: form {info['form']} obstacle_form {info['obstacle_form']} nranks {info['nranks']} "
          f"row_table_lds {info['row_table_lds']} resident {info['resident_groups']} needed {info['needed_groups']}")
    assert info["form"] == sc.step_form, info
    assert info["obstacle_form"] == "grid", info
    assert info["nranks"] == max(1, sc.local_group), info
    assert_same_state(g, make_oracle(sc), check_unexplored=True, label=sc.name)

"""Solution paths resampled at a fixed period, the parts that need no GPU
(include/sbmp/tree_resample.h):

  sbmp_tree_resample_batch_host   the host twin (resample_paths_host) against the model of
                                  tests/tree_resample_model.py, bit for bit: states as uint32,
                                  times as uint64, edges and counts exactly
  the float64 audit               every sample against the float64 linear interpolation, at
                                  fraction alpha / dt, between the Euler states j and j + 1 of
                                  tests/f64_model.py, within twice its first-order bound; the
                                  audit fails on two deliberately wrong rules
  tests/tree_resample_host_main.cpp   the twin over exact-size heap arrays, built stand-alone with
                                  -fsanitize=address,undefined and run once
  the ABI                         the new symbols, the refused arguments
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import f64_model
import tree_recheck_cases as tc
import tree_resample_cases as rc
from conftest import ROOT, bits
from tree_paths_model import BROKEN, DEEP, NONE, OK, trace_model
from tree_resample_model import WRONG_RULES, TooManySamples, assert_same_resample, resample_model

INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def host(case, nodes, period, depthBound=0, **kw):
    from cudasbmp_amd import tree_resample_batch
    return tree_resample_batch(case.state, case.ctrl, case.parent, nodes, period, depthBound=depthBound, device=False,
                               **dict(rc.params_of(case), **kw))


def model(case, nodes, period, depthBound=0, **kw):
    return resample_model(case.state, case.ctrl, case.parent, nodes, period, depth_bound=depthBound,
                          **dict(rc.params_of(case), **kw))


def check(case, nodes, period, depthBound=0, **kw):
    want = model(case, nodes, period, depthBound, details=True, **kw)
    got = host(case, nodes, period, depthBound, **kw)
    assert_same_resample(got, want, label=f"{case.name} host vs model")
    return got, want


def test_many_requests_whose_samples_pass_one_grid_sweep():
    """The case tests/test_gpu_tree_resample.py holds k_path_resample's later sweeps to: the twin
    equals the model on it, and the total lies where the case says."""
    case, nodes, period = rc.many_requests()
    _, want = check(case, nodes, period)
    total = int(want["offsets"][-1])
    assert rc.SWEEP + 1000 <= total <= 1.2 * rc.SWEEP
    assert {NONE, BROKEN, OK} <= set(want["status"].tolist()) and 650 <= len(nodes) <= 750


# ---------------------------------------------------------------- grown trees
@pytest.mark.parametrize("period", rc.PERIODS, ids=rc.PERIOD_IDS)
@pytest.mark.parametrize("g", tc.GROWN, ids=tc.GROWN_IDS)
def test_host_resample_of_a_grown_tree_is_the_model(g, period):
    case = tc.grown(*g)
    got, want = check(case, rc.nodes_of(case), period)
    assert np.all(got["status"] == OK) and len(got["times"]) > 1000
    # every path: times ascend from 0 to T, the last sample is the node as stored
    for i, node in enumerate(rc.nodes_of(case)):
        a, b = got["offsets"][i], got["offsets"][i + 1]
        assert b - a >= 2 and got["times"][a] == 0.0 and np.all(np.diff(got["times"][a:b]) >= 0)
        assert got["edges"][b - 1] == node and np.array_equal(bits(got["states"][b - 1]), bits(case.state[node]))
    grid = want["from"] >= 0
    assert grid.sum() > len(grid) // 2 and want["j"][grid].max() == g[2] - 1


# ---------------------------------------------------------------- the float64 audit
AUDITED = [("car", 1.0, 10), ("car", 1.3, 13), ("point", 1.0, 10), ("car", 1.0, 1)]
AUDITED_IDS = [f"{a}-L{L:g}-D{D}" for a, L, D in AUDITED]


@functools.lru_cache(maxsize=None)
def _f64_steps(g):
    """(R, D + 1, 4) float64 states and first-order bounds after 0 .. D Euler steps of every row's
    edge (row 0: unused), from tests/f64_model.py run with numDisc = j and duration j / D, as the
    trace audit runs it."""
    agent, L, D = g
    case = tc.grown(*g)
    R = len(case.parent)
    par = case.state[np.maximum(case.parent, 0)]
    states = np.zeros((R, D + 1, 4))
    bounds = np.zeros((R, D + 1, 4))
    states[:, 0] = par
    none = np.zeros((0, 4))
    for j in range(1, D + 1):
        c = case.ctrl[:, :3].astype(np.float64)
        c[:, 2] = c[:, 2] * j / D
        if agent == "point":
            s, _, b, _ = f64_model.replay_point(par, c, j, L, np.inf, np.inf, none)
        else:
            s, _, b, _ = f64_model.replay_car(par, c, j, L, np.inf, np.inf, none)
        states[:, j], bounds[:, j] = s, b
    return states, bounds


def _audit(g, rule=""):
    """The worst err / bound over every grid sample and component of the tree's three periods.
    In real arithmetic a step of alpha from Euler state j is the linear interpolation between the
    states j and j + 1 at alpha / dt (every update is linear in the step length).  The allowance
    is the float64 model's first-order bound after j + 1 steps: each of its terms is proportional
    to the step length or to the state's magnitude, so it covers a last step of alpha <= dt."""
    case = tc.grown(*g)
    states, bounds = _f64_steps(g)
    worst = 0.0
    for period in rc.PERIODS:
        m = model(case, rc.nodes_of(case), period, details=True, rule=rule)
        grid = m["from"] >= 0
        e, j = m["edges"][grid].astype(np.int64), m["j"][grid]
        assert np.all(m["dt"][grid] > 0)
        # the fraction from the right rule's alpha, whatever the model under audit did with it
        right = m if not rule else model(case, rc.nodes_of(case), period, details=True)
        f = right["alpha"][grid].astype(np.float64) / right["dt"][grid].astype(np.float64)
        want = states[e, j] + f[:, None] * (states[e, j + 1] - states[e, j])
        err = np.abs(m["states"][grid].astype(np.float64) - want)
        bound = bounds[e, j + 1]
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("g", AUDITED, ids=AUDITED_IDS)
def test_every_sample_within_twice_the_float64_bound(g):
    worst = _audit(g)
    print(f"{g}: worst err / bound {worst:.3f}")
    assert worst <= 2.0, worst


@pytest.mark.parametrize("rule", WRONG_RULES)
def test_the_audit_notices_a_wrong_rule(rule):
    assert _audit(tc.MAIN, rule=rule) > 2.0


# ---------------------------------------------------------------- crafted chains
@pytest.mark.parametrize("period", rc.PERIODS[:2], ids=rc.PERIOD_IDS[:2])
@pytest.mark.parametrize("L", rc.CHAIN_LENGTHS)
def test_chains_of_every_size_class(L, period):
    case = rc.chain(L)
    got, want = check(case, [L - 1], period)
    T = 0.0
    for _ in range(L - 1):
        T += float(np.float32(0.07))
    assert got["status"].tolist() == [OK] and got["counts"].tolist() == [int(np.floor(T / period)) + 2]
    if L == 1:
        assert got["counts"].tolist() == [2] and got["times"].tolist() == [0.0, 0.0] and got["edges"].tolist() == [0, 0]
        assert np.array_equal(bits(got["states"]), bits(case.state[[0, 0]]))
    else:
        assert period < 0.07 and set(got["edges"].tolist()) == set(range(1, L))   # every edge holds a grid time


@pytest.mark.parametrize("agent", ["car", "point"])
def test_power_of_two_durations_land_on_step_and_edge_boundaries(agent):
    case = rc.pow2(7, agent)
    D, last = 8, 6
    steps, _ = trace_model(case.state, case.ctrl, case.parent, **case.params)
    stored = case.state if agent == "car" else case.state * np.array([1, 1, 0, 0], np.float32)
    assert float(np.float32(1.0) / np.float32(D)) == 0.125
    # every grid time a step boundary: sample m is the state after m % 8 steps of edge m // 8 + 1
    got, want = check(case, [last], 0.125)
    assert got["counts"].tolist() == [last * D + 2] and np.all(want["alpha"] == 0.0)
    for m in range(last * D):
        k, j = m // D + 1, m % D
        assert got["edges"][m] == k and want["j"][m] == j and got["times"][m] == m * 0.125
        landed = stored[k - 1] if j == 0 else steps[k, j - 1]
        assert np.all(got["states"][m] == landed), (m, got["states"][m], landed)
    assert got["times"][-2:].tolist() == [6.0, 6.0] and got["edges"][-2:].tolist() == [last, last]
    # every grid time an edge boundary: sample m is row m as stored
    got, want = check(case, [last], 1.0)
    assert got["counts"].tolist() == [last + 2] and got["edges"].tolist() == [1, 2, 3, 4, 5, 6, 6, 6]
    assert np.all(want["j"] == 0) and np.all(want["alpha"] == 0.0)
    assert np.all(got["states"][:last] == stored[:last])
    assert np.array_equal(bits(got["states"][last:]), bits(case.state[[last, last]]))


def test_a_period_longer_than_the_path_gives_the_root_and_the_node():
    case = rc.chain(65)
    got, _ = check(case, [64], 100.0)
    assert got["counts"].tolist() == [2] and got["edges"].tolist() == [1, 64]
    assert np.all(got["states"][0] == case.state[0]) and np.array_equal(bits(got["states"][1]), bits(case.state[64]))
    assert got["times"][0] == 0.0 and got["times"][1] == float(np.sum(np.full(64, np.float32(0.07), np.float64)))


@pytest.mark.parametrize("period", [0.05, 0.013, 0.3, 1e-3])
def test_bad_durations_add_no_time_and_are_never_selected(period):
    case = rc.bad_durations()
    node = len(case.parent) - 1
    got, want = check(case, [node], period)
    T = 0.0
    for d in (np.float32(1e-45), np.float32(0.3), np.float32(0.2), np.float32(0.25), np.float32(0.4)):
        T += float(d)
    assert got["times"][-1] == T and got["counts"].tolist() == [int(np.floor(T / period)) + 2]
    assert not np.isin(got["edges"], rc.BAD_ROWS).any()
    # the denormal edge: dt == 0, so j = numDisc - 1 and alpha = (float)tau; only t = 0 lies in it
    assert got["edges"][0] == rc.DENORMAL_ROW and got["edges"][1] != rc.DENORMAL_ROW
    assert want["dt"][0] == 0.0 and want["j"][0] == case.params["numDisc"] - 1 and want["alpha"][0] == 0.0
    assert np.all(got["states"][0] == case.state[0])
    assert np.isfinite(got["states"]).all()


def test_a_last_grid_time_that_rounds_past_the_path_is_an_end_sample():
    case = rc.rounding()
    T, p, m = float(rc.ROUNDING_DURATION), rc.ROUNDING_PERIOD, rc.ROUNDING_GRID
    assert int(np.floor(T / p)) == m and m * p > T           # the case's own precondition
    got, _ = check(case, [1], p)
    assert got["counts"].tolist() == [m + 2]
    assert got["times"][m] == T and got["times"][m + 1] == T and got["times"][m - 1] < T
    assert got["edges"][m - 1:].tolist() == [1, 1, 1]
    assert np.array_equal(bits(got["states"][m:]), bits(case.state[[1, 1]]))


# ---------------------------------------------------------------- statuses, requests
def test_none_broken_and_deep_requests_get_no_samples():
    case = tc.parent_case("minus1")
    busiest = tc.busiest_row(*tc.MAIN)
    child = int(np.flatnonzero(tc.grown(*tc.MAIN).parent == busiest)[0])
    nodes = np.array([7, -1, busiest, 9, child, -1, 0], np.int32)
    got, _ = check(case, nodes, 0.05)
    assert got["status"].tolist() == [OK, NONE, BROKEN, OK, BROKEN, NONE, OK]
    assert np.all(got["counts"][[1, 2, 4, 5]] == 0) and np.all(got["counts"][[0, 3, 6]] >= 2)
    assert got["edges"][got["offsets"][3 + 1] - 1] == 9 and got["edges"][-1] == 0
    deep = rc.chain(65)
    got, _ = check(deep, [64, 63, 64], 0.05, depthBound=64)
    assert got["status"].tolist() == [DEEP, OK, DEEP] and got["counts"][[0, 2]].tolist() == [0, 0]
    assert got["offsets"].tolist() == [0, 0, got["counts"][1], got["counts"][1]]


def test_duplicates_any_order_and_no_requests():
    case = tc.grown(*tc.MAIN)
    R = len(case.parent)
    nodes = np.array([R - 1, 0, 77, R - 1, 77, 0], np.int32)
    got, _ = check(case, nodes, 0.013)
    o = got["offsets"]
    for a, b in ((0, 3), (2, 4), (1, 5)):
        assert got["states"][o[a]:o[a + 1]].tobytes() == got["states"][o[b]:o[b + 1]].tobytes()
        assert got["times"][o[a]:o[a + 1]].tobytes() == got["times"][o[b]:o[b + 1]].tobytes()
    empty = host(case, np.zeros(0, np.int32), 0.05)
    assert len(empty["counts"]) == 0 and empty["offsets"].tolist() == [0] and empty["states"].shape == (0, 4)


def test_the_point_agent_on_a_crafted_chain():
    case = rc.pow2(7, "point")
    got, _ = check(case, [6, 3], 0.3)
    assert np.all(got["states"][:, 2:] == 0.0) and got["counts"].tolist() == [22, 12]


# ---------------------------------------------------------------- the stand-alone program
def test_twin_standalone_under_sanitizers(tmp_path):
    """The twin over exact-size heap arrays for the crafted chains, as its own program under
    AddressSanitizer and UBSan."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_resample_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_resample_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# ---------------------------------------------------------------- the ABI
def test_library_exports_the_resample_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_resample_paths", "sbmp_tree_resample_batch", "sbmp_tree_resample_batch_host"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert L.sbmp_abi_version() == 1


def test_refused_arguments():
    from cudasbmp_amd import _native as nat
    case = rc.chain(4)
    L = nat.lib()
    counts, status = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    states, edges, times = np.zeros((64, 4), np.float32), np.zeros(64, np.int32), np.zeros(64, np.float64)
    total = ctypes.c_longlong(-5)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def args(**changes):
        a = nat.TreePathsArgs()
        a.state, a.ctrl, a.parent = case.state.ctypes.data, case.ctrl.ctypes.data, case.parent.ctypes.data
        a.rows, a.depthBound, a.agent, a.numDisc, a.agentLength = 4, 0, 0, 10, 1.0
        for k, v in changes.items():
            setattr(a, k, v)
        return a

    def call(nodes, period=0.05, capacity=64, out=True, a=None, tot=total):
        n = np.array(nodes, np.int32)
        return L.sbmp_tree_resample_batch_host(ctypes.byref(a or args()), vp(n) if len(n) else None, len(n), period,
                                               vp(counts), vp(status), vp(states) if out else None,
                                               vp(edges) if out else None, vp(times) if out else None, capacity,
                                               ctypes.byref(tot) if tot is not None else None)

    T = 3 * float(np.float32(0.07))
    n3 = int(np.floor(T / 0.05)) + 2
    assert call([3, 0, -1]) == 0 and total.value == n3 + 2 and counts[:3].tolist() == [n3, 2, 0]
    for bad in (0.0, -0.05, float("nan"), float("inf"), -float("inf")):
        assert call([3], period=bad) == INVALID
    assert call([-2]) == INVALID and call([4]) == INVALID and call([3, 4]) == INVALID
    total.value = -1
    assert call([3, 3], capacity=2 * n3 - 1) == INVALID and total.value == 2 * n3    # *total is set all the same
    assert call([3, 3], capacity=0, out=False) == 0 and total.value == 2 * n3       # the sizing call
    assert call([3, 3], capacity=2 * n3) == 0
    assert call([]) == 0 and total.value == 0                                        # count 0: a no-op
    assert call([], period=0.0) == INVALID
    assert call([3], tot=None) == INVALID
    assert call([3], a=args(rows=0)) == INVALID and call([3], a=args(parent=None)) == INVALID
    assert call([3], a=args(numDisc=0)) == INVALID and call([3], a=args(agent=2)) == INVALID
    assert L.sbmp_tree_resample_batch_host(None, None, 0, 0.05, None, None, None, None, None, 0,
                                           ctypes.byref(total)) == INVALID
    # T / period at the bound: 2^31 - 2 and beyond is refused, just below it is sized
    big = T / (2.0 ** 31 - 1.5)
    assert T / big >= 2.0 ** 31 - 2 and call([3], period=big, out=False) == INVALID
    below = T / (2.0 ** 31 - 2.5)
    assert T / below < 2.0 ** 31 - 2
    assert call([3], period=below, out=False, capacity=0) == 0 and total.value == 2 ** 31 - 3 + 2
    assert call([3], period=5e-324, out=False) == INVALID
    with pytest.raises(TooManySamples):
        resample_model(case.state, case.ctrl, case.parent, [3], big)

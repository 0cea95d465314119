"""Paths and traces of a grown tree, the parts that need no GPU (include/sbmp/tree_paths.h):

  sbmp_tree_trace_batch_host   the host twin (trace_rows_host over traceCarControls /
  sbmp_tree_paths_batch_host   tracePointControls; path_rows_host) against the model of
                               tests/tree_paths_model.py (exact float32 numpy + an explicit
                               parent walk), bit for bit
  the float64 audit            every step of the twin against tests/f64_model.py run with
                               numDisc = j and duration j / D, within twice its first-order bound
  the cases' preconditions     asserted, so that no case goes vacuous
  tests/tree_paths_host_main.cpp   the twins over exact-size heap arrays with crafted parents and
                               depthBound at the boundary, built stand-alone with
                               -fsanitize=address,undefined and run once
  the ABI                      the new symbols, the refused arguments
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
from conftest import ROOT
from tree_paths_model import (BROKEN, DEEP, FREE, NONE, OK, ORPHAN, STALE, assert_same_paths, assert_same_trace,
                              paths_model, trace_model)
from tree_recheck_model import depths

AUDITED = [("car", 1.0, 10), ("car", 1.3, 13), ("point", 1.0, 10), ("car", 1.0, 1)]
AUDITED_IDS = [f"{a}-L{L:g}-D{D}" for a, L, D in AUDITED]
INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def trace_params(case):
    return {k: case.params[k] for k in ("numDisc", "agentLength", "agent")}


def host_trace(case, rows=None):
    from cudasbmp_amd import tree_trace_batch
    return tree_trace_batch(case.state, case.ctrl, case.parent, rows, device=False, **trace_params(case))


def host_paths(case, nodes, depthBound=0):
    from cudasbmp_amd import tree_paths_batch
    return tree_paths_batch(case.state, case.ctrl, case.parent, nodes, depthBound=depthBound, device=False)


@functools.lru_cache(maxsize=None)
def model_trace(g):
    case = tc.grown(*g)
    return trace_model(case.state, case.ctrl, case.parent, **case.params)


# ---------------------------------------------------------------- grown trees
@pytest.mark.parametrize("g", tc.GROWN, ids=tc.GROWN_IDS)
def test_host_trace_of_a_grown_tree_is_the_model_and_ends_on_the_rows(g):
    case = tc.grown(*g)
    steps, status = host_trace(case)
    assert_same_trace((steps, status), model_trace(g), label=case.name)
    assert len(status) == len(case.parent) > 1000 and np.all(status == FREE)
    assert np.array_equal(np.ascontiguousarray(steps[:, -1]).view(np.uint32), case.state.view(np.uint32))
    assert depths(case.parent).max() >= 3


def _audit(g, steps, alter=frozenset()):
    """The worst err / bound over every row > 0, step and component."""
    agent, L, D = g
    case = tc.grown(*g)
    par = case.state[case.parent[1:]]
    worst = 0.0
    for j in range(1, D + 1):
        c = case.ctrl[1:, :3].astype(np.float64)
        c[:, 2] = c[:, 2] * j / D
        if agent == "point":
            want, valid, bound, _ = f64_model.replay_point(par, c, j, L, np.inf, np.inf, np.zeros((0, 4)))
        else:
            want, valid, bound, _ = f64_model.replay_car(par, c, j, L, np.inf, np.inf, np.zeros((0, 4)), alter=alter)
        assert alter or valid.all()   # x > 0 is all that is left of the workspace test; an alteration may cross it
        err = np.abs(steps[1:, j - 1].astype(np.float64) - want)
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("g", AUDITED, ids=AUDITED_IDS)
def test_every_step_within_twice_the_float64_bound(g):
    steps, _ = host_trace(tc.grown(*g))
    worst = _audit(g, steps)
    print(f"{g}: worst err / bound {worst:.3f}")
    assert worst <= 2.0, worst


@pytest.mark.parametrize("alter", ["theta-before-x", "dt-over-steps-plus-one"])
def test_the_audit_notices_an_altered_order(alter):
    g = tc.MAIN
    steps, _ = host_trace(tc.grown(*g))
    assert _audit(g, steps, alter=frozenset({alter})) > 2.0


# ---------------------------------------------------------------- crafted rows
@pytest.mark.parametrize("column", [0, 2], ids=["x", "theta"])
def test_a_moved_state_is_stale_on_that_row_only(column):
    case = tc.stale_case(column)
    r = tc.busiest_row(*tc.MAIN)
    steps, status = host_trace(case)
    assert_same_trace((steps, status), trace_model(case.state, case.ctrl, case.parent, **case.params), label=case.name)
    # the row itself, and its children: their traces start from the moved state (one that happens
    # to end on the same bits stays FREE); no other row reads the moved floats
    stale = np.flatnonzero(status == STALE)
    children = np.flatnonzero(case.parent == r)
    assert status[r] == STALE and len(children) and np.all(np.isin(stale, np.append(children, r)))
    assert (status == FREE).sum() == len(status) - len(stale)
    own, _ = model_trace(tc.MAIN)
    others = np.setdiff1d(np.arange(len(status)), np.append(children, r))
    assert np.array_equal(np.ascontiguousarray(steps[others]).view(np.uint32), own[others].view(np.uint32))


def _below(parent, rows):
    """Rows whose chain passes through one of `rows` (those rows included)."""
    below = np.zeros(len(parent), bool)
    below[list(rows)] = True
    for q in range(1, len(parent)):
        if not below[q]:
            below[q] = below[parent[q]]
    return below


@pytest.mark.parametrize("kind", tc.PARENT_KINDS)
def test_crafted_parents_break_paths_and_orphan_traces(kind):
    case = tc.parent_case(kind)
    own = tc.grown(*tc.MAIN)
    rows = tc.parent_rows()
    R = len(case.parent)
    _, status = host_trace(case)
    assert np.array_equal(np.flatnonzero(status == ORPHAN), np.array(sorted(rows)))
    assert (status == FREE).sum() == R - 4
    every = np.arange(R, dtype=np.int32)
    got = host_paths(case, every)
    assert_same_paths(got, paths_model(case.state, case.ctrl, case.parent, every), label=case.name)
    below = _below(own.parent, rows)
    busiest = tc.busiest_row(*tc.MAIN)
    child = int(np.flatnonzero(own.parent == busiest)[0])
    assert got["status"][busiest] == BROKEN and got["status"][child] == BROKEN and below.sum() > 4
    assert np.array_equal(got["status"] == BROKEN, below) and np.all(got["status"][~below] == OK)
    assert np.all(got["lengths"][below] == 0) and np.all(got["lengths"][~below] == depths(own.parent)[~below] + 1)


def test_rows_counted_and_never_written_are_broken_and_orphan():
    case = tc.d6_case()
    R = len(case.parent)
    assert R == 1000 and np.all(case.parent[993:] == -1)
    steps, status = host_trace(case)
    assert_same_trace((steps, status), trace_model(case.state, case.ctrl, case.parent, **case.params), label="d6")
    assert np.all(status[993:] == ORPHAN) and not np.any(status[:993] == ORPHAN)
    assert np.array_equal(np.ascontiguousarray(steps[993:]).view(np.uint32),
                          np.repeat(case.state[993:, None, :], case.params["numDisc"], axis=1).view(np.uint32))
    every = np.arange(R, dtype=np.int32)
    got = host_paths(case, every)
    assert_same_paths(got, paths_model(case.state, case.ctrl, case.parent, every), label="d6")
    assert np.all(got["status"][993:] == BROKEN) and np.all(got["status"][:993] == OK)


# ---------------------------------------------------------------- depth, requests
@pytest.mark.parametrize("depth", tc.CHAIN_DEPTHS)
def test_depth_bound_at_the_chain_length_and_one_less(depth):
    case = tc.chain_case(depth, "last")
    rows = depth + 1
    got = host_paths(case, [depth], depthBound=rows)
    assert_same_paths(got, paths_model(case.state, case.ctrl, case.parent, [depth], rows), label=f"chain {depth}")
    assert got["status"].tolist() == [OK] and np.array_equal(got["rows"], np.arange(rows))
    short = host_paths(case, [depth], depthBound=rows - 1)
    assert_same_paths(short, paths_model(case.state, case.ctrl, case.parent, [depth], rows - 1), label="one less")
    assert short["status"].tolist() == [DEEP] and short["lengths"].tolist() == [0] and len(short["rows"]) == 0


def test_requests_none_root_duplicates_and_any_order():
    case = tc.grown(*tc.MAIN)
    R = len(case.parent)
    deep = int(np.argmax(depths(case.parent)))
    nodes = np.array([-1, 0, deep, 7, deep, R - 1, -1, 0, 3], np.int32)
    got = host_paths(case, nodes)
    assert_same_paths(got, paths_model(case.state, case.ctrl, case.parent, nodes), label="requests")
    assert got["status"][[0, 6]].tolist() == [NONE, NONE] and got["lengths"][[0, 1, 6, 7]].tolist() == [0, 1, 0, 1]
    assert got["lengths"][2] == got["lengths"][4] == depths(case.parent)[deep] + 1 >= 4
    a, b = got["offsets"][2], got["offsets"][4]
    n = got["lengths"][2]
    assert np.array_equal(got["rows"][a:a + n], got["rows"][b:b + n]) and got["rows"][a] == 0 and got["rows"][a + n - 1] == deep
    empty = host_paths(case, np.zeros(0, np.int32))
    assert len(empty["lengths"]) == 0 and empty["offsets"].tolist() == [0] and len(empty["rows"]) == 0
    # a listed trace: duplicates and any order
    rows = np.array([deep, 0, 7, deep, R - 1], np.int32)
    assert_same_trace(host_trace(case, rows), trace_model(case.state, case.ctrl, case.parent, rows, **case.params),
                      label="listed rows")


def test_twins_standalone_under_sanitizers(tmp_path):
    """The twins over exact-size heap arrays with every crafted parent and depthBound at the
    boundary, as their own program under AddressSanitizer and UBSan."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_paths_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_paths_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# ---------------------------------------------------------------- the ABI
def test_library_exports_the_paths_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_solution_paths", "sbmp_kgmt_trace_rows", "sbmp_tree_paths_batch", "sbmp_tree_paths_batch_host",
              "sbmp_tree_trace_batch", "sbmp_tree_trace_batch_host"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert L.sbmp_abi_version() == 1
    assert (nat.SBMP_PATH_OK, nat.SBMP_PATH_NONE, nat.SBMP_PATH_BROKEN, nat.SBMP_PATH_DEEP) == (OK, NONE, BROKEN, DEEP)
    assert ctypes.sizeof(nat.TreePathsArgs) == 48


def test_refused_arguments():
    from cudasbmp_amd import _native as nat
    case = tc.chain_case(3, "last")
    L = nat.lib()
    lengths, status = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    rows, samples, costs = np.zeros(16, np.int32), np.zeros((16, 7), np.float32), np.zeros(16, np.float32)
    steps, rstatus = np.zeros((10, 4, 4), np.float32), np.zeros(4, np.uint8)
    total = ctypes.c_longlong(-5)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def args(**changes):
        a = nat.TreePathsArgs()
        a.state, a.ctrl, a.parent = case.state.ctypes.data, case.ctrl.ctypes.data, case.parent.ctypes.data
        a.rows, a.depthBound, a.agent, a.numDisc, a.agentLength = 4, 0, 0, 10, 1.0
        for k, v in changes.items():
            setattr(a, k, v)
        return a

    def paths(nodes, capacity=16, out=True, a=None, tot=total):
        n = np.array(nodes, np.int32)
        return L.sbmp_tree_paths_batch_host(ctypes.byref(a or args()), vp(n) if len(n) else None, len(n), vp(lengths),
                                            vp(status), vp(rows) if out else None, vp(samples) if out else None,
                                            vp(costs) if out else None, capacity, ctypes.byref(tot) if tot is not None else None)

    assert paths([3, 0, -1]) == 0 and total.value == 5 and lengths[:3].tolist() == [4, 1, 0]
    assert paths([-2]) == INVALID and paths([4]) == INVALID and paths([3, 4]) == INVALID
    assert paths([3, 3], capacity=7) == INVALID and total.value == 8          # *total is set all the same
    assert paths([3, 3], capacity=0, out=False) == 0 and total.value == 8     # the sizing call
    assert paths([]) == 0 and total.value == 0                                # count 0: a no-op
    assert paths([3], tot=None) == INVALID
    assert paths([3], a=args(rows=0)) == INVALID and paths([3], a=args(parent=None)) == INVALID
    assert L.sbmp_tree_paths_batch_host(ctypes.byref(args()), None, 2, vp(lengths), vp(status), None, None, None, 0,
                                        ctypes.byref(total)) == INVALID
    assert L.sbmp_tree_paths_batch_host(None, None, 0, None, None, None, None, None, 0, ctypes.byref(total)) == INVALID

    def trace(rows_, count, a=None, out=steps):
        r = np.array(rows_, np.int32) if rows_ is not None else None
        return L.sbmp_tree_trace_batch_host(ctypes.byref(a or args()), vp(r) if r is not None else None, count,
                                            vp(out) if out is not None else None, vp(rstatus))

    assert trace(None, 4) == 0 and rstatus.tolist() == [FREE] * 4
    assert trace([3, 0, 3, 1], 4) == 0
    assert trace(None, 0) == 0                                                # count 0: a no-op
    assert trace(None, 5) == INVALID                                          # more than the tree holds
    assert trace([4], 1) == INVALID and trace([-1], 1) == INVALID
    assert trace(None, 4, out=None) == INVALID
    assert trace(None, -1) == INVALID
    assert trace(None, 4, a=args(numDisc=0)) == INVALID and trace(None, 4, a=args(agent=2)) == INVALID

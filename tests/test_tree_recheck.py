"""The tree re-check, the parts that need no GPU (include/sbmp/tree_recheck.h):

  sbmp_tree_recheck_batch_host   the host twin (one ascending loop over propagateCarControls /
                                 propagatePointControls) against the model of
                                 tests/tree_recheck_model.py (the CPU oracle's replay + numpy)
                                 on every case of tests/tree_recheck_cases.py, byte for byte
  the cases' preconditions       asserted on the model itself, so that no case goes vacuous
  tests/tree_recheck_host_main.cpp   the twin over exact-size heap arrays with crafted parents,
                                 built stand-alone with -fsanitize=address,undefined and run once
  the ABI                        the new symbols, the refused arguments
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tree_recheck_cases as tc
from conftest import ROOT
from tree_recheck_model import (BLOCKED, CUT, FREE, ORPHAN, STALE, assert_same_recheck, depths, descendants)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def host(case):
    from cudasbmp_amd import tree_recheck_batch
    return tree_recheck_batch(case.state, case.ctrl, case.parent, case.boxes, device=False, **case.params)


@pytest.mark.parametrize("build", [b for _, b in tc.CPU_CASES], ids=tc.CPU_IDS)
def test_host_twin_matches_model(build):
    case = build()
    status, summary, _ = case.model
    assert_same_recheck(host(case), (status, summary), label=case.name)


@pytest.mark.parametrize("g", tc.GROWN, ids=tc.GROWN_IDS)
def test_own_boxes_leave_every_row_alive(g):
    case = tc.grown(*g)
    status, summary, alive = case.model
    R = len(case.parent)
    assert R > 1000 and depths(case.parent).max() >= 3
    assert np.all(status == FREE) and alive.all()
    assert summary == dict(rows=R, alive=R, blocked=0, stale=0, orphan=0, cut=0, firstDead=-1)


@pytest.mark.parametrize("g", tc.GROWN, ids=tc.GROWN_IDS)
def test_blocked_row_cuts_its_subtree(g):
    case = tc.blocked(*g)
    r = tc.busiest_row(*g)
    status, summary, alive = case.model
    assert depths(case.parent)[r] >= 2
    assert status[r] == BLOCKED
    assert summary["cut"] >= 1 and summary["alive"] >= 2
    assert summary["firstDead"] <= r
    below = np.flatnonzero(case.parent == r)
    assert len(below) and not alive[below].any()


@pytest.mark.parametrize("g", [tc.MAIN, ("point", 1.0, 10), ("car", 1.3, 13)], ids=["car", "point", "car-L1.3-D13"])
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_verdicts_flip_on_one_float(g, axis):
    r = tc.edge_row(*g, axis)
    want = {"box": {"at": FREE, "in": BLOCKED, "out": FREE}, "wall": {"at": BLOCKED, "in": FREE, "out": BLOCKED}}
    for kind in ("box", "wall"):
        for variant in ("at", "in", "out"):
            case = tc.edge_case(*g, axis, kind, variant)
            assert case.model[0][r] & 0x7f == want[kind][variant], (kind, variant)
            assert host(case)[0][r] == case.model[0][r], (kind, variant)


@pytest.mark.parametrize("kind", tc.PARENT_KINDS)
def test_crafted_parents_are_orphans(kind):
    case = tc.parent_case(kind)
    own = tc.grown(*tc.MAIN)
    status = host(case)[0]
    rows = tc.parent_rows()
    assert len(set(rows)) == 4 and rows[:2] == (1, 5) and rows[3] == len(case.parent) - 1
    for r in rows:
        assert status[r] == ORPHAN
        below = np.flatnonzero(own.parent == r)
        assert np.all(status[below] == (FREE | CUT))
    assert sum(descendants(own.parent)[r] for r in rows) > 0
    below = np.zeros(len(status), bool)                            # rows under a crafted row
    for q in range(1, len(status)):
        below[q] = below[own.parent[q]] or own.parent[q] in rows
    below[list(rows)] = False
    assert np.array_equal(status == (FREE | CUT), below)           # the subtrees, and nothing else, are cut
    assert (status == ORPHAN).sum() == 4


@pytest.mark.parametrize("column", [0, 2], ids=["x", "theta"])
def test_a_moved_state_is_stale(column):
    case = tc.stale_case(column)
    r = tc.busiest_row(*tc.MAIN)
    status, summary, alive = case.model
    assert status[r] == STALE and summary["cut"] >= 1
    # every row below r is dead: its children replay from the moved state (STALE or BLOCKED
    # themselves, or CUT where the replay happens to end on the same bits), theirs are CUT
    dead = np.zeros(len(alive), bool)
    dead[r] = True
    for q in range(r + 1, len(alive)):
        dead[q] = dead[case.parent[q]]
    assert not alive[dead].any() and alive[~dead].all()


def test_reference_clear_tree_holds_rows_never_written():
    case = tc.d6_case()
    status, summary, _ = case.model
    assert summary["orphan"] + summary["stale"] >= 1, summary
    assert np.all(case.parent[status == ORPHAN] == -1)


@pytest.mark.parametrize("depth", tc.CHAIN_DEPTHS)
def test_chain_blocked_at_either_end(depth):
    first, last = tc.chain_case(depth, "first").model[1], tc.chain_case(depth, "last").model[1]
    assert first == dict(rows=depth + 1, alive=1, blocked=1, stale=0, orphan=0, cut=depth - 1, firstDead=1)
    assert last == dict(rows=depth + 1, alive=depth, blocked=1, stale=0, orphan=0, cut=0, firstDead=depth)


def test_box_lists_block_some_rows_and_a_nan_box_blocks_all():
    assert tc.boxes_case(0).model[1]["alive"] == tc.SMALL
    for n in tc.BOX_COUNTS[3:]:
        s = tc.boxes_case(n).model[1]
        assert s["blocked"] >= 1 and s["alive"] >= 2, (n, s)
    for n in (5, 600):
        s = tc.nan_case(n).model[1]
        assert s["blocked"] + s["cut"] == tc.SMALL - 1 and s["alive"] == 1, (n, s)


def test_twin_standalone_under_sanitizers(tmp_path):
    """The twin over exact-size heap arrays with every crafted parent, as its own program under
    AddressSanitizer and UBSan: an orphan's parent word must never be used as an index."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_recheck_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_recheck_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_library_exports_the_recheck_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_recheck_tree", "sbmp_kgmt_query_goals_alive", "sbmp_tree_recheck_batch",
              "sbmp_tree_recheck_batch_host", "sbmp_tree_query_alive_batch", "sbmp_tree_query_alive_batch_host"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert ctypes.sizeof(nat.TreeRecheck) == 28
    assert (nat.SBMP_ROW_FREE, nat.SBMP_ROW_ORPHAN, nat.SBMP_ROW_BLOCKED, nat.SBMP_ROW_STALE, nat.SBMP_ROW_CUT) == \
        (FREE, ORPHAN, BLOCKED, STALE, CUT)


def test_refused_arguments():
    from cudasbmp_amd import _native as nat
    case = tc.chain_case(3, "last")
    INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT
    out = nat.TreeRecheck()
    status = np.zeros(4, np.uint8)

    def call(**changes):
        a = nat.TreeRecheckArgs()
        a.state, a.ctrl, a.parent = case.state.ctypes.data, case.ctrl.ctypes.data, case.parent.ctypes.data
        a.rows, a.depthBound, a.agent, a.numDisc = 4, 0, 0, 10
        a.agentLength, a.width, a.height = 1.0, 20.0, 20.0
        a.obstacles, a.obstaclesCount = case.boxes.ctypes.data, 1
        for k, v in changes.items():
            setattr(a, k, v)
        return nat.lib().sbmp_tree_recheck_batch_host(ctypes.byref(a), status.ctypes.data_as(ctypes.c_void_p),
                                                      ctypes.byref(out))

    assert call() == 0 and out.rows == 4
    assert call(obstaclesCount=-1) == INVALID
    assert call(obstacles=None) == INVALID               # a NULL list with count > 0
    assert call(obstacles=None, obstaclesCount=0) == 0
    assert call(rows=0) == INVALID
    assert call(numDisc=0) == INVALID
    assert call(agent=2) == INVALID
    assert call(parent=None) == INVALID
    assert nat.lib().sbmp_tree_recheck_batch_host(None, None, ctypes.byref(out)) == INVALID

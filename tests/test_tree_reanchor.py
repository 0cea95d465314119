"""The re-anchoring rule without a GPU (include/sbmp/tree_reanchor.h).

  the host twin                     sbmp_tree_reanchor_batch_host equals the independent model
                                    (tests/tree_reanchor_model.py: the CPU oracle's replay level by
                                    level + numpy) bit for bit on the whole table
                                    (tests/tree_reanchor_cases.py)
  coverage                          the model alone shows that the displaced grown trees reach the
                                    three outcomes the table names
  tests/tree_reanchor_host_main.cpp the twin over exact-size heap arrays, built stand-alone with
                                    -fsanitize=address,undefined and run once
  the ABI                           the new symbols and the refused arguments
The capacity protocol of sbmp_kgmt_reanchor_tree needs a planner handle, so it is held in
tests/test_gpu_tree_reanchor.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tree_recheck_cases as tc
import tree_reanchor_cases as rc
from conftest import ROOT
from tree_recheck_model import depths
from tree_reanchor_model import assert_same_reanchor


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def host(c, **over):
    from cudasbmp_amd import tree_reanchor_batch
    kw = dict(c.params, depth_bound=c.bound, device=False)
    kw.update(over)
    return tree_reanchor_batch(c.state, c.ctrl, c.parent, c.s0, c.boxes, **kw)


@pytest.mark.parametrize("build", [b for _, b in rc.CASES], ids=rc.CASE_IDS)
def test_host_twin_is_the_model(build):
    c = build()
    assert_same_reanchor(host(c), c.model, label=f"{c.name} host vs model")   # the twin reads no bound


@pytest.mark.parametrize("g", tc.GROWN, ids=tc.GROWN_IDS)
def test_the_displaced_grown_trees_reach_every_outcome(g):
    """By the model alone, with s0 = the stored root + (+0.05, -0.03, +0.02 rad, 0): at least one
    alive row at depth >= 3, one blocked row and one cut row on each grown tree.  The counts
    (rows: alive / alive at depth >= 3 / blocked / cut):
        car   L 1   D 1   48,761: 42,379 / 10,374 / 866 / 5,516
        car   L 1   D 10  21,298: 19,448 /  2,945 / 116 / 1,734
        car   L 1   D 13  20,546: 19,850 /  3,406 / 133 /   563
        car   L 1.3 D 1   45,547: 38,871 /  6,866 / 859 / 5,817
        car   L 1.3 D 10  20,086: 19,616 /  3,046 / 116 /   354
        car   L 1.3 D 13  19,941: 19,317 /  2,776 / 100 /   524
        point L 1   D 1   25,424: 25,381 /  4,785 /  26 /    17
        point L 1   D 10  25,714: 25,581 /  4,984 /  21 /   112
        point L 1   D 13  27,327: 27,304 /  6,707 /  19 /     4
    With s0 = the stored root bits, and one ulp off in x, every row of every tree stays alive."""
    c = rc.grown(*g, "moved")
    _, alive, _, s = c.model
    deep = int((alive & (depths(c.parent) >= 3)).sum())
    print(f"{c.name}: rows {s['rows']} alive {s['alive']} deep {deep} blocked {s['blocked']} cut {s['cut']}")
    assert deep >= 1 and s["blocked"] >= 1 and s["cut"] >= 1 and s["orphan"] == 0 and s["levels"] >= 4
    same = rc.grown(*g, "same").model
    assert same[1].all() and np.array_equal(same[0][1:].view(np.uint32), c.state[1:].view(np.uint32))   # invariant I1


def test_the_table_reaches_what_it_names():
    far = rc.far_parent()
    d = depths(far.parent)
    assert (np.diff(d) < 0).any() and far.model[3]["levels"] == int(d.max()) + 1 >= 40
    assert far.model[3]["blocked"] >= 1 and far.model[3]["cut"] >= 1 and far.model[1][d >= 3].any()
    for k in tc.PARENT_KINDS:
        c = rc.parent_case(k)
        _, alive, status, s = c.model
        assert s["orphan"] == 4 and (status[list(tc.parent_rows())] == 1).all()
        busiest = tc.busiest_row(*tc.MAIN)
        below = np.flatnonzero((c.parent == busiest) & (np.arange(len(c.parent)) > busiest))   # `self` names itself
        assert len(below) and (status[below] == 0x80).all() and not alive[below].any()
    b = rc.blocked()
    assert b.model[2][tc.busiest_row(*tc.MAIN)] == 2 and b.model[3]["cut"] > rc.grown(*tc.MAIN, "moved").model[3]["cut"]
    assert rc.wall().model[3]["blocked"] > rc.grown(*tc.MAIN, "moved").model[3]["blocked"]
    for d_ in tc.CHAIN_DEPTHS:
        assert rc.chain(d_, "last").model[3]["levels"] == d_ + 1
    assert rc.chain(257, "first", "same").model[3]["cut"] == 256
    assert rc.star(rc.STAR_ROWS).model[3]["levels"] == 2
    assert rc.nan_case(5).model[3]["alive"] == 1


def test_the_table_passes_one_sweep_and_the_lds_seam():
    """By the model alone: what the cases past a sweep and round the 2,048 LDS depth counters reach."""
    S = rc.SWEEP
    assert S == 256 * 8 * 256 and rc.LDS_DEPTHS == 2048
    s = rc.big_star().model[3]
    assert (s["rows"], s["levels"], s["cut"]) == (S + 77, 2, 0) and s["blocked"] > 1000        # level 1: S + 76 rows
    rec = rc.recursive(0)
    _, alive, status, s = rec.model
    # all of 500,165 alive, 5,668 blocked, 18,532 cut occur; this tree has no orphan (every parent is a lower row)
    assert (s["alive"], s["blocked"], s["cut"], s["orphan"], s["levels"]) == (500165, 5668, 18532, 0, 33)
    assert alive[S:].any() and (status[S:] != 0).any()
    d = depths(rec.parent)
    assert np.bincount(d).max() < S and d[S:].max() > 4 and (np.diff(d) < 0).any()
    assert rc.hist_depths(S + 77) == S + 77 > rc.LDS_DEPTHS and rc.hist_depths(S + 77, 64) == 65 > s["levels"]
    assert rc.recursive(64).parent is rec.parent and rc.recursive(64).bound == 64
    for bound in (4, 9):
        c = rc.short_bound_past_sweep(bound)
        d = depths(c.parent)
        assert c.model[3]["levels"] == 10 and np.flatnonzero(d > 4).min() == S + 72 and c.refused == (bound == 4)
        assert c.bound == bound and (1 << 2) < d.max() == 9 <= (1 << 4)
    assert [rc.hist_depths(n) for n in rc.SEAM_ROWS] == [2047, 2048, 2049] and rc.hist_depths(2049, 2048) == 2049
    for e in rc.LONG_CHAIN_EDGES:
        c = rc.long_chain(e)
        s = c.model[3]
        assert (s["rows"], s["alive"], s["levels"]) == (e + 1, e + 1, e + 1)
        assert depths(c.parent)[-1] == rc.hist_depths(e + 1) - 1 == e       # a row on the last counter
    assert rc.hist_depths(2047) <= rc.LDS_DEPTHS == rc.hist_depths(2048) < rc.hist_depths(2049)
    assert rc.hist_depths(2048, 1025) == 2048 and (1 << 11) >= 2047 > (1 << 10) and rc.hist_depths(2048, 1024) == 1025
    assert not rc.long_chain(2047, 1025).refused and rc.long_chain(2047, 1024, True).refused


def test_twin_standalone_under_sanitizers(tmp_path):
    """The twin over exact-size heap arrays, chains, stars, random and crafted parents, as its own
    program under AddressSanitizer and UBSan."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_reanchor_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_reanchor_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_library_exports_the_reanchor_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_reanchor_tree", "sbmp_kgmt_replan_from", "sbmp_tree_reanchor_batch",
              "sbmp_tree_reanchor_batch_host"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert L.sbmp_abi_version() == 1
    import cudasbmp_amd
    assert "tree_reanchor_batch" in cudasbmp_amd.__all__
    assert hasattr(cudasbmp_amd.KGMT, "reanchor") and hasattr(cudasbmp_amd.KGMT, "replan_from")


@pytest.mark.parametrize("bad", list(rc.BAD_ROOTS), ids=list(rc.BAD_ROOTS))
def test_a_non_finite_root_is_refused(bad):
    from cudasbmp_amd import SbmpError
    c = rc.chain(8, "last")
    with pytest.raises(SbmpError) as e:
        host(rc.RCase(c.name, c.state, c.ctrl, c.parent, c.boxes, c.params, np.array(rc.BAD_ROOTS[bad], np.float32)))
    assert e.value.status == 1


def test_refused_arguments():
    from cudasbmp_amd import SbmpError, tree_reanchor_batch, _native as nat
    c = rc.chain(8, "last")
    host(c)
    for over in (dict(numDisc=0), dict(agent="point", numDisc=-3)):
        with pytest.raises(SbmpError) as e:
            host(c, **over)
        assert e.value.status == 1, over
    with pytest.raises(SbmpError) as e:
        tree_reanchor_batch(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32), c.s0,
                            c.boxes, device=False)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        tree_reanchor_batch(c.state, c.ctrl[:-1], c.parent, c.s0, c.boxes, device=False)
    with pytest.raises(ValueError):
        tree_reanchor_batch(c.state, c.ctrl, c.parent, c.s0[:3], c.boxes, device=False)
    L = nat.lib()
    s = nat.TreeReanchor()
    s0 = np.ascontiguousarray(c.s0, np.float32)
    a = nat.TreeRecheckArgs()
    a.state, a.ctrl, a.parent = c.state.ctypes.data, c.ctrl.ctypes.data, c.parent.ctypes.data
    a.rows, a.agent, a.numDisc, a.agentLength, a.width, a.height = len(c.parent), nat.SBMP_AGENT_CAR, 10, 1.0, 20.0, 20.0
    p0 = s0.ctypes.data_as(ctypes.c_void_p)
    assert L.sbmp_tree_reanchor_batch_host(None, p0, None, None, None, ctypes.byref(s)) == 1
    assert L.sbmp_tree_reanchor_batch_host(ctypes.byref(a), p0, None, None, None, None) == 1
    assert L.sbmp_tree_reanchor_batch_host(ctypes.byref(a), None, None, None, None, ctypes.byref(s)) == 1
    a.obstaclesCount = 3                                           # a NULL list with a count
    assert L.sbmp_tree_reanchor_batch_host(ctypes.byref(a), p0, None, None, None, ctypes.byref(s)) == 1
    a.obstaclesCount = -1
    assert L.sbmp_tree_reanchor_batch_host(ctypes.byref(a), p0, None, None, None, ctypes.byref(s)) == 1
    a.obstaclesCount = 0
    a.agent = 7
    assert L.sbmp_tree_reanchor_batch_host(ctypes.byref(a), p0, None, None, None, ctypes.byref(s)) == 1
    a.agent = nat.SBMP_AGENT_CAR
    # every output may be NULL: the summary alone
    assert L.sbmp_tree_reanchor_batch_host(ctypes.byref(a), p0, None, None, None, ctypes.byref(s)) == 0
    assert s.rows == len(c.parent) and s.levels == len(c.parent) and s.alive == s.rows
    # a handle-level call without a handle
    assert L.sbmp_kgmt_reanchor_tree(None, 0, p0, None, 0, None, None, None, None, None, 0, ctypes.byref(s)) == 1

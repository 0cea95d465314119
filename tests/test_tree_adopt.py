"""The adoption rule without a GPU (include/sbmp/tree_adopt.h).

  the host twin                  sbmp_tree_adopt_tables_host equals the independent numpy model
                                 (tests/tree_adopt_model.py) bit for bit on the whole table
                                 (tests/tree_adopt_cases.py)
  the root                       a one-row table is what the reference's root seeding leaves
                                 (KGMT.cu:85-97, written out in the model module from those lines)
  tests/tree_adopt_host_main.cpp the twin over exact-size heap arrays, built stand-alone with
                                 -fsanitize=address,undefined and run once
  the ABI                        the new symbols and the refused arguments
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tree_adopt_cases as ac
import tree_adopt_model as model
from conftest import ROOT


def host(c, **over):
    from cudasbmp_amd import tree_adopt_tables
    kw = dict(c.grid, goal=c.goal, frontier_from=c.frontier_from, device=False)
    kw.update(over)
    return tree_adopt_tables(c.state, **kw)


@pytest.mark.parametrize("cid", ac.CASE_IDS)
def test_host_twin_is_the_model(cid):
    c = ac.case(cid)
    model.same_tables(host(c), c.model, label=f"{c.name} host vs model")


def test_the_twin_reaches_every_seam_of_the_table():
    """What the host twin answers on the table shows that the table reaches each seam it names."""
    cs = ac.cases()
    assert tuple(cs) == ac.CASE_IDS
    twin = {k: host(c) for k, c in cs.items()}
    s = {k: t["summary"] for k, t in twin.items()}
    assert {c.rows for c in cs.values()} >= set(ac.ROW_COUNTS) | {ac.ONE_CELL_ROWS}
    one = twin["one-cell-disc"]
    assert one["R1"].max() == ac.ONE_CELL_ROWS > 0xffff and one["R1Cov"].sum() == 1 and s["one-cell-disc"]["goalRow"] == 0
    assert s["nonfinite-disc"]["nonFinite"] > s["nonfinite-disc"]["frontierNonFinite"] > 0
    assert s["outside-nogoal"]["outOfGrid"] >= 12
    # on a line and one ulp under it are different cells; one ulp over it is the line's cell
    assert np.count_nonzero(twin["r1-lines-nogoal"]["R1"]) >= 31
    # the quotient rounds up onto the line although the real quotient lies below it
    st, w, c = ac.round_up_case()
    R1Size = model.sizes(w, 16, 8)[0]
    assert np.float32(st[0, 0] / R1Size) == c and float(st[0, 0]) / float(R1Size) < c
    from cudasbmp_amd import tree_adopt_tables
    up_ = tree_adopt_tables(st[:1], width=w, height=20.0, N=16, n=8, device=False)
    assert int(np.flatnonzero(up_["R1"])[0]) % 16 == c
    # the disc at equality is outside (sqrt(d2) < r), one ulp more takes the row in; the lowest row wins
    eq, upc, dn = s["goal-edge-disc"], s["goal-edge-up-disc"], s["goal-edge-down-disc"]
    assert upc["goalRow"] == 2 and eq["goalRow"] > 2 and dn["goalRow"] >= eq["goalRow"]
    assert s["goal-radius-zero-disc"]["goalRow"] == -1
    assert all(v["goalRow"] == -1 for k, v in s.items() if k.endswith("-nogoal"))
    assert [s[f"frontier-{k}-disc"]["gLo"] for k in ("0", "last", "R")] == [0, 299, 300]
    assert {(c.N, c.n) for c in cs.values()} >= {(1, 1), (1, 16), (16, 1), (16, 8), (16, 16)}
    assert any(c.width != c.height for c in cs.values())


def test_the_table_passes_one_sweep():
    """The cases past a sweep are what they are named for, by the model and by the twin."""
    S = ac.SWEEP
    assert S == 256 * 8 * 256
    for name, R in ac.PAST_SWEEP:
        c = ac.case(name + "-disc")
        inside = np.flatnonzero(model.in_goal(c.state[:, 0], c.state[:, 1], c.goal))
        assert c.rows == R > S and inside[0] < S and all(((inside >= k * S) & (inside < (k + 1) * S)).sum() > 1000
                                                         for k in range(R // S))
        assert inside[-1] == R - 1 >= R // S * S                  # and the last, partial sweep holds one
        assert c.model["summary"]["goalRow"] == host(c)["summary"]["goalRow"] == inside[0]
        assert (c.model["R1"] > 1000).all() and c.model["R1Cov"].min() == 64
    c = ac.case("goal-past-sweep-disc")
    assert c.rows == S + 77 and c.model["summary"]["goalRow"] == host(c)["summary"]["goalRow"] == S + 40
    c = ac.case("goal-both-sweeps-disc")
    inside = np.flatnonzero(model.in_goal(c.state[:, 0], c.state[:, 1], c.goal))
    assert inside.tolist() == list(ac.GOAL_BOTH) + [r + S for r in ac.GOAL_BOTH]
    assert len({r // 64 for r in ac.GOAL_BOTH}) == 3 and len({r // 256 for r in ac.GOAL_BOTH}) == 2
    assert c.model["summary"]["goalRow"] == host(c)["summary"]["goalRow"] == min(ac.GOAL_BOTH)
    c = ac.case("counters-past-sweep-nogoal")
    s = host(c)["summary"]
    bad = ~np.isfinite(c.state).all(axis=1)
    assert np.flatnonzero(bad).tolist() == [S + r for r in ac.COUNTERS_NONFINITE] and c.frontier_from == S + 10
    assert (s["nonFinite"], s["frontierNonFinite"], s["outOfGrid"]) == (7, 4, 9) and s == c.model["summary"]
    first = model.tables(c.state[:S], c.width, c.N, c.n)["summary"]           # the first sweep counts nothing
    assert (first["nonFinite"], first["outOfGrid"]) == (0, 0)


@pytest.mark.parametrize("x, y", [(5.0, 5.0), (0.0, 0.0), (19.999, 0.1), (1.25, 2.5), (20.0, 3.0), (-0.5, 3.0),
                                  (3.0, float("nan")), (float("inf"), 1.0), (17.3, 17.3)])
@pytest.mark.parametrize("grid", [dict(width=20.0, N=16, n=8), dict(width=17.3, N=16, n=3), dict(width=20.0, N=1, n=1)])
def test_one_row_is_the_reference_root_seeding(x, y, grid):
    from cudasbmp_amd import tree_adopt_tables
    st = np.array([[x, y, 0.1, 0.2]], dtype=np.float32)
    got = tree_adopt_tables(st, height=20.0, goal=None, device=False, **grid)
    model.same_tables({k: v for k, v in got.items() if k != "summary"},
                      model.seed_root_tables(x, y, grid["width"], grid["N"], grid["n"]), label=f"root ({x}, {y})")


def test_twin_standalone_under_sanitizers(tmp_path):
    """The twin over exact-size heap arrays, every grid shape and the special floats, as its own
    program under AddressSanitizer and UBSan."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_adopt_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_adopt_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_library_exports_the_adopt_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_adopt_tree", "sbmp_kgmt_replan", "sbmp_tree_adopt_tables", "sbmp_tree_adopt_tables_host"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert L.sbmp_abi_version() == 1


def test_refused_arguments():
    from cudasbmp_amd import SbmpError, tree_adopt_tables, _native as nat
    st = ac.random_rows(10, 1)
    ok = dict(width=20.0, height=20.0, N=16, n=8, goal=None, frontier_from=0, device=False)
    tree_adopt_tables(st, **ok)
    bad = [dict(frontier_from=-1), dict(frontier_from=11), dict(N=0), dict(N=17), dict(n=0), dict(n=17),
           dict(width=0.0), dict(width=-1.0), dict(width=float("nan")), dict(goal=(float("nan"), 1.0, 0.5)),
           dict(goal=(1.0, float("inf"), 0.5))]
    for over in bad:
        with pytest.raises(SbmpError) as e:
            tree_adopt_tables(st, **dict(ok, **over))
        assert e.value.status == 1, over
    with pytest.raises(SbmpError) as e:
        tree_adopt_tables(np.zeros((0, 4), dtype=np.float32), **ok)
    assert e.value.status == 1
    # NULL args and NULL out
    L = nat.lib()
    s = nat.TreeAdopt()
    assert L.sbmp_tree_adopt_tables_host(None, None, None, None, None, None, None, ctypes.byref(s)) == 1
    a = nat.TreeAdoptTablesArgs()
    a.state, a.rows, a.width, a.height, a.N, a.n = st.ctypes.data, 10, 20.0, 20.0, 16, 8
    assert L.sbmp_tree_adopt_tables_host(ctypes.byref(a), None, None, None, None, None, None, None) == 1
    # frontier_from == rows is the empty frontier, an answer
    assert tree_adopt_tables(st, **dict(ok, frontier_from=10))["summary"]["gLo"] == 10

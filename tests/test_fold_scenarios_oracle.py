"""Family K (tests/fold_scenarios.py) on the CPU oracle alone: every committed scenario reaches
what it is there for.  Taken from the oracle's iter_logs() and its unexplored() after every step:

  (a) iterations t > window with S(t) < S(t - window) and S(t) % 8 != 0: ring row t % window
      holds the keys of t - window at and past S(t), and the 8-key piece at S(t) straddles it.
      At least 2 in every scenario; at least 4 with 3 residues of S mod 8 in the best one.
  (b) in at least one of them a slot of [S(t), S(t - window)) holds, from iteration t - window,
      a child inside the workspace: a fold without the S mask would change a count.
  (c) at least 128 iterations execute (two windows).
  (d) R2Valid + R2Invalid has more than 1,000 nonzero cells at the end: the tables are not
      compared vacuously.

Measured: K-base 2 such iterations (66, 68; residues 5, 6), 14,840 nonzero cells; K-best 5
(96, 97, 101, 105, 107; residues 1, 4, 6), 15,394 cells; K-best-n11 4 (66, 97, 100, 130;
residues 2, 4, 5), 27,653 of 30,976 cells; K-best-n3 (samplesPerIteration 128) 4 (66, 69, 79, 82;
residues 4, 5, 6, 7), 1,976 of 2,304 cells; in every one of them (b) holds.
"""
import pytest

import fold_scenarios as fs


@pytest.fixture(scope="module")
def window(oracle_lib):
    from cudasbmp_amd import fold_r2_info
    w = fold_r2_info(256)["window"]
    assert w == fs.WINDOW   # the scenarios were chosen for this window
    return w


@pytest.mark.parametrize("name", fs.IDS)
def test_scenario_reaches_the_stale_part_of_the_ring(name, window):
    sc = fs.BY_NAME[name]
    c = fs.coverage(sc)
    print(name, c)
    assert len(c["stale"]) >= max(2, sc.min_stale), c                     # (a)
    assert len(c["residues"]) >= sc.min_residues and 0 not in c["residues"], c
    assert all(t > window for t in c["stale"])
    assert len(c["counting"]) >= 1 and set(c["counting"]) <= set(c["stale"]), c   # (b)
    assert c["executed"] >= 2 * window, c                                 # (c)
    assert c["nonzero_cells"] > 1000 and c["nR2"] == sc.nR2, c            # (d)
    assert c["S_min"] < c["S_max"]


def test_the_table_holds_the_base_the_best_and_the_key_log_sizes():
    from cudasbmp_amd import fold_r2_info
    assert fs.BASE.min_stale == 2 and fs.BEST.min_stale >= 4 and fs.BEST.min_residues >= 3
    sizes = {s.n for s in fs.SCENARIOS}
    assert {3, 8, 11} <= sizes
    assert all(s.nR2 <= fold_r2_info(256)["maxR2"] for s in fs.SCENARIOS)   # every one folds its key log

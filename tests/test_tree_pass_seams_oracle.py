"""The cases that take the newer tree passes past one grid sweep and to their seams, proven on
the CPU alone: a correct pass gives the model's answer on every one of them, and each of a list
of wrong passes, written here in numpy, is caught.  (tests/test_tree_query_cases_oracle.py does
the same for the masked goal query.)

Each pass is stated a second time, the way its kernels work and not the way its model does, with
switches that each break it the way a grid-stride kernel could be broken.  SWEEP = 524,288 rows
is one sweep of a grid of 8 workgroups of 256 lanes on each of 256 CUs.

  extract (tree_extract.hip): pointer jumping for the members, a count per tile, the offsets in
  rounds of roundTiles tiles with a carried base, the numbering inside a tile, the gather
    past-sweep-dropped    rows >= SWEEP are never members
    tile-round-dropped    the tiles >= 2,048 (a second round of k_extract_count / _number) are never
                          taken: their rows are in no count and get no number
    offsets-base-lost     tileOff restarts at 0 in every round of k_extract_offsets
    offsets-base-once     every later round adds the first round's total only
    below-first-sweep     `below` counted over rows < SWEEP only
  adopt (tree_adopt.hip): the cells of tests/tree_adopt_model.py, the counters, the goal row as
  the lowest over the waves of each wave's first inside row, the copy into the planner's tree
    past-sweep-dropped    rows >= SWEEP in no table and no counter
    goal-first-sweep-only the goal row taken over rows < SWEEP only
    goal-last-met         a wave keeps the highest inside row it meets (across rounds: the later one)
    copy-past-sweep-dropped   rows >= SWEEP never copied into the planner's tree (the planner-level
                          case of tests/test_gpu_tree_adopt.py alone looks at the copy)
  reanchor (tree_reanchor.hip): pointer jumping for the depths, the short-bound flag, the depth
  counts, the level offsets, the levels in turn through the CPU oracle's replay
    past-sweep-dropped    rows >= SWEEP keep depth 0: they are orphans
    level-past-sweep-dropped  the entries >= SWEEP of a level are not replayed (their outputs stay unwritten)
    last-lds-depth-dropped    the count of depth `depths - 1` is lost where the counters are in LDS
    lds-at-2049           2,049 depths still counted in the 2,048 LDS counters: the count of depth 2,048 is lost
    short-flag-first-sweep    the short-bound flag raised by rows < SWEEP only
    short-flag-lost       the short-bound flag never raised: an answer where the call must be refused
    lds-counts-not-flushed    where the depths fit the LDS counters, no workgroup adds its counts to the global ones
    global-counts-lost    where they do not fit, the adds never reach the global counters
                          (these two show on which side of `depths <= 2,048` each seam case lies)
  resample (tree_resample.hip): every sample's request by bisecting the sample offsets, its edge
  by bisecting the request's clock
    past-sweep-dropped    samples >= SWEEP never written
    request-0-past-sweep  the samples >= SWEEP attributed to request 0

A wrong pass is caught by a case when its answer differs from the expected one in any field.  A
wrong pass whose kernel counterpart would throw ("the level offsets do not cover the rows", "the
tile offsets and the summary disagree") answers with that error in place of a summary, which
differs.  CAUGHT_BY names, for every wrong pass, cases built to catch it, and each must; over the
whole table every wrong pass is caught and no new case is idle.
"""
import functools

import numpy as np
import pytest

import tree_adopt_cases as ac
import tree_adopt_model as amodel
import tree_extract_cases as xc
import tree_reanchor_cases as rc
import tree_resample_cases as sc
from tree_paths_model import OK, path_of
from tree_query_cases import SWEEP
from tree_recheck_model import BLOCKED, CUT, FREE, ORPHAN, planner_config
from tree_reanchor_model import summary_of
from tree_resample_model import clock_of, count_of, resample_model


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def _same_arrays(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _table(cases, wrongs, caught) -> dict:
    return {(w, n): caught(n, w) for n in cases for w in wrongs}


def _check_wrong(w, table, cases, caught_by):
    by = [n for n in cases if table[w, n]]
    print(w, "caught by", by)
    assert by, f"nothing catches {w}"
    missed = [n for n in caught_by[w] if not table[w, n]]
    assert not missed, f"{w} passes {missed}, which were built to catch it"


def _check_table(table, cases, wrongs, caught_by):
    caught = [w for w in wrongs if any(table[w, n] for n in cases)]
    idle = [n for n in cases if not any(table[w, n] for w in wrongs)]
    print(f"{len(caught)} of {len(wrongs)} wrong passes caught; idle cases: {idle}")
    assert set(caught_by) == set(wrongs) and len(caught) == len(wrongs)
    assert not idle, f"cases that catch no wrong pass: {idle}"


# ================================================================ extract
X_CASES = tuple(f"rows-{w}{m}" for w in xc.PAST_SWEEP for m in ("", "-masked")) + (
    "rows-tiles+1-packed-by-mask", "root-past-sweep", "root-past-sweep-masked")
X_WRONG = ("past-sweep-dropped", "tile-round-dropped", "offsets-base-lost", "offsets-base-once", "below-first-sweep")
X_CAUGHT_BY = {
    "past-sweep-dropped": X_CASES,
    "tile-round-dropped": ("rows-tiles+1", "rows-tiles+1-masked", "rows-tiles+1-packed-by-mask"),
    "offsets-base-lost": tuple(n for n in X_CASES if not n.startswith("root-")),
    "offsets-base-once": tuple(n for n in X_CASES if not n.startswith("root-")),
    "below-first-sweep": ("root-past-sweep", "root-past-sweep-masked"),
}
X_ARRAYS = ("parent", "origin", "newRow")


@functools.lru_cache(maxsize=None)
def _members(name):
    """(member, kept) by k_extract_mark and pointer jumping to the fixed point (the kernels take
    ceil(log2 rows) passes; a pass after the fixed point changes nothing)."""
    c = xc.case(name)
    R = c.rows
    r = np.arange(R, dtype=np.int64)
    kept = np.ones(R, bool) if c.keep is None else c.keep != 0
    p = c.parent.astype(np.int64)
    above = r > c.root
    usable = above & kept & (p >= 0) & (p < r)
    dead = (r < c.root) | ~kept | (above & ~usable)
    anc = np.where(dead | ~above, r, p)
    while True:
        dead = dead | dead[anc]
        nxt = anc[anc]
        if np.array_equal(nxt, anc):
            break
        anc = nxt
    return ~dead, kept


def extract(name, wrong=()) -> dict:
    c = xc.case(name)
    tile, round_rows = xc.layout()
    P = round_rows // tile
    R, root = c.rows, c.root
    member, kept = _members(name)
    member = member.copy()
    r = np.arange(R, dtype=np.int64)
    if "past-sweep-dropped" in wrong:
        member[SWEEP:] = False
    taken = np.ones(R, bool)                      # the rows whose tile a workgroup takes
    if "tile-round-dropped" in wrong:
        taken[xc.SWEEP_TILES * tile:] = False
    # k_extract_count: the classes and one count per tile
    below = (r < root) & (r < SWEEP if "below-first-sweep" in wrong else True)
    acc = {"kept": int((member & taken).sum()), "below": int((below & taken).sum()),
           "masked": int((~(r < root) & ~kept & taken).sum()),
           "detached": int((~(r < root) & kept & ~member & taken).sum())}
    starts = np.arange(0, R, tile)
    count = np.add.reduceat((member & taken).astype(np.int64), starts)
    # k_extract_offsets: rounds of P tiles, `base` carried
    off = np.zeros(len(count), np.int64)
    base, first_total = 0, 0
    for k, t0 in enumerate(range(0, len(count), P)):
        part = count[t0:t0 + P]
        if "offsets-base-lost" in wrong:
            base = 0
        elif "offsets-base-once" in wrong and k >= 1:
            base = first_total
        off[t0:t0 + P] = base + np.cumsum(part) - part
        base += int(part.sum())
        if k == 0:
            first_total = base
    K = base
    if K != acc["kept"]:
        return {"error": "the tile offsets and the summary disagree"}
    # k_extract_number: the tile's offset and the members before the row in its tile
    cs = np.cumsum(member & taken)
    before_tile = np.concatenate([[0], cs[tile - 1::tile]])[:len(count)]
    newRow = np.where(member & taken, off[r // tile] + cs - 1 - before_tile[r // tile], -1).astype(np.int32)
    # k_extract_gather
    src = np.flatnonzero((newRow >= 0) & (newRow < K))
    origin = np.full(K, -1, np.int32)
    origin[newRow[src]] = src
    parent = np.full(K, -1, np.int32)
    old = np.where(src == root, root, c.parent[src]).astype(np.int64)
    parent[newRow[src]] = np.where(src == root, -1, newRow[np.clip(old, 0, R - 1)])
    out = {"parent": parent, "origin": origin, "newRow": newRow,
           "summary": dict(acc, rows=R, root=root, rootCost=c.ctrl[root, 3])}
    if not wrong:
        out["state"], out["ctrl"] = c.state[origin], c.ctrl[origin]
    return out


def _extract_caught(name, w) -> bool:
    got, want = extract(name, (w,)), xc.case(name).model
    if "error" in got:
        return True
    return any(got["summary"][k] != want["summary"][k] for k in ("rows", "kept", "below", "masked", "detached", "root")) \
        or not all(_same_arrays(got[k], want[k]) for k in X_ARRAYS)


@pytest.mark.parametrize("name", X_CASES)
def test_extract_the_true_pass_is_the_model(name):
    from tree_extract_model import assert_same_extract
    assert_same_extract(extract(name), xc.case(name).model, label=name)


@pytest.fixture(scope="module")
def x_table():
    return _table(X_CASES, X_WRONG, _extract_caught)


@pytest.mark.parametrize("w", X_WRONG)
def test_extract_wrong_pass_is_caught(w, x_table):
    _check_wrong(w, x_table, X_CASES, X_CAUGHT_BY)


def test_extract_every_wrong_pass_is_caught_and_no_case_is_idle(x_table):
    _check_table(x_table, X_CASES, X_WRONG, X_CAUGHT_BY)
    two_rounds = ("rows-round+1", "rows-round+1-masked")        # the older table stops at two rounds of the offsets
    assert not any(_extract_caught(n, "offsets-base-once") for n in two_rounds)
    assert all(_extract_caught(n, "offsets-base-lost") for n in two_rounds)


# ================================================================ adopt
A_STEP = tuple(n + s for n in [p for p, _ in ac.PAST_SWEEP] + ["goal-past-sweep", "goal-both-sweeps", "counters-past-sweep"]
               for s in ("-nogoal", "-disc"))
A_PLANNER = "planner-sweep+77"
A_CASES = A_STEP + (A_PLANNER,)
A_WRONG = ("past-sweep-dropped", "goal-first-sweep-only", "goal-last-met", "copy-past-sweep-dropped")
A_CAUGHT_BY = {
    "past-sweep-dropped": A_CASES,
    "goal-first-sweep-only": ("goal-past-sweep-disc",),
    "goal-last-met": ("goal-both-sweeps-disc",),
    "copy-past-sweep-dropped": (A_PLANNER,),
}
A_FAR_GOAL = (-5.0, -5.0, 0.5)


def _adopt_inputs(name):
    """(state, grid, goal, frontier_from, the rows to copy or None)"""
    if name == A_PLANNER:
        state, ctrl, parent, f = ac.planner_past_sweep()
        return state, ac.DEMO_GRID, A_FAR_GOAL, f, (state, ctrl, parent)
    c = ac.case(name)
    return c.state, c.grid, c.goal, c.frontier_from, None


@functools.lru_cache(maxsize=None)
def _adopt_expect(name):
    state, grid, goal, f, rows = _adopt_inputs(name)
    t = amodel.tables(state, grid["width"], grid["N"], grid["n"], goal, f) if rows else ac.case(name).model
    return t, rows


def adopt(name, wrong=()) -> dict:
    state, grid, goal, f, rows = _adopt_inputs(name)
    N, n = grid["N"], grid["n"]
    R = len(state)
    seen = min(R, SWEEP) if "past-sweep-dropped" in wrong else R
    st = state[:seen]
    # k_adopt_scan: cells, counters, the goal row
    r1, r2 = amodel.cells(st[:, 0], st[:, 1], grid["width"], N, n)
    bad = ~np.isfinite(st).all(axis=1)
    inside = np.flatnonzero(amodel.in_goal(st[:, 0], st[:, 1], goal))
    if "goal-first-sweep-only" in wrong:
        inside = inside[inside < SWEEP]
    goal_row = -1
    if len(inside):
        wave = (inside % SWEEP) // 64                     # a wave's rows: its 64 lanes, one sweep apart
        order = np.lexsort((inside, wave))
        w_sorted, rows_sorted = wave[order], inside[order]
        first = np.concatenate([[True], w_sorted[1:] != w_sorted[:-1]])
        last = np.concatenate([w_sorted[1:] != w_sorted[:-1], [True]])
        goal_row = int(rows_sorted[last if "goal-last-met" in wrong else first].min())
    summary = {"rows": R, "nonFinite": int(bad.sum()), "frontierNonFinite": int(bad[f:].sum()),
               "outOfGrid": int(((r1 < 0) | (r2 < 0)).sum()), "goalRow": goal_row, "treeSize": R, "gLo": int(f)}
    # k_adopt_seed and k_adopt_tables
    nR1, nn = N * N, n * n
    count = np.bincount(r1[r1 >= 0], minlength=nR1).astype(np.int32)
    bits = np.zeros((nR1 * nn + 31) // 32 * 32, np.uint8)
    bits[r2[r2 >= 0]] = 1
    out = {"R1": count, "R1Avail": (count > 0).astype(np.int32), "R1Valid": count.copy(), "R1Invalid": np.zeros(nR1, np.int32),
           "R1Cov": bits[:nR1 * nn].reshape(nR1, nn).sum(axis=1).astype(np.int32),
           "R2bits": np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).ravel(),
           "summary": summary}
    if rows:
        copied = min(R, SWEEP) if "copy-past-sweep-dropped" in wrong or "past-sweep-dropped" in wrong else R
        out["tree"] = [np.concatenate([a[:copied], np.zeros_like(a[copied:])]) for a in rows]
    return out


def _adopt_caught(name, w) -> bool:
    got = adopt(name, (w,))
    want, rows = _adopt_expect(name)
    if got["summary"] != want["summary"] or not all(_same_arrays(got[k], want[k]) for k in amodel.R1_TABLES + ("R2bits",)):
        return True
    return bool(rows) and not all(_same_arrays(g, r) for g, r in zip(got["tree"], rows))


@pytest.mark.parametrize("name", A_CASES)
def test_adopt_the_true_pass_is_the_model(name):
    got = adopt(name)
    want, rows = _adopt_expect(name)
    amodel.same_tables(got, want, label=name)
    assert not rows or all(_same_arrays(g, r) for g, r in zip(got["tree"], rows))


@pytest.fixture(scope="module")
def a_table():
    return _table(A_CASES, A_WRONG, _adopt_caught)


@pytest.mark.parametrize("w", A_WRONG)
def test_adopt_wrong_pass_is_caught(w, a_table):
    _check_wrong(w, a_table, A_CASES, A_CAUGHT_BY)


def test_adopt_every_wrong_pass_is_caught_and_no_case_is_idle(a_table):
    _check_table(a_table, A_CASES, A_WRONG, A_CAUGHT_BY)
    assert set(A_STEP) <= set(ac.CASE_IDS)
    # the counters lie past the sweep only: dropped rows lose every one of them
    got = adopt("counters-past-sweep-nogoal", ("past-sweep-dropped",))["summary"]
    assert (got["nonFinite"], got["frontierNonFinite"], got["outOfGrid"]) == (0, 0, 0)
    # the lowest inside row shares its wave with higher ones, in its round and in the next
    assert adopt("goal-both-sweeps-disc", ("goal-last-met",))["summary"]["goalRow"] == ac.GOAL_BOTH[2] + SWEEP


# ================================================================ reanchor
R_BUILD = dict(rc.past_sweep_cases())
R_CASES = tuple(R_BUILD)
R_WRONG = ("past-sweep-dropped", "level-past-sweep-dropped", "last-lds-depth-dropped", "lds-at-2049", "short-flag-first-sweep",
           "short-flag-lost", "lds-counts-not-flushed", "global-counts-lost")
R_CAUGHT_BY = {
    "past-sweep-dropped": ("star-sweep+77", "recursive-sweep+77", "recursive-sweep+77-bound-64", "short-bound-past-sweep-4",
                           "short-bound-past-sweep-9"),
    "level-past-sweep-dropped": ("star-sweep+77", "short-bound-past-sweep-9"),
    "last-lds-depth-dropped": ("chain-2046", "chain-2047", "chain-2047-bound-1025"),
    "lds-at-2049": ("chain-2048",),
    "short-flag-first-sweep": ("short-bound-past-sweep-4",),
    "short-flag-lost": ("short-bound-past-sweep-4", "chain-2047-bound-1024"),
    "lds-counts-not-flushed": ("rows-2047", "rows-2048", "chain-2046", "chain-2047", "chain-2047-bound-1025",
                               "recursive-sweep+77-bound-64"),
    "global-counts-lost": ("rows-2049", "rows-2049-bound-2048", "chain-2048", "recursive-sweep+77", "star-sweep+77"),
}
UNWRITTEN = 0xEE        # a status byte no launch wrote
REFUSED = {"refused": "depthBound"}


def _reanchor_plan(c, wrong=()):
    """Everything before the levels: REFUSED, an error, or (hop, off, levels)."""
    R = len(c.parent)
    r = np.arange(R, dtype=np.int64)
    p = c.parent.astype(np.int64)
    usable = (p >= 0) & (p < r)
    if "past-sweep-dropped" in wrong:
        usable[SWEEP:] = False
    anc, hop = np.where(usable, p, r), usable.astype(np.int64)
    bound = min(c.bound, R) if c.bound > 0 else R
    passes = max(1, int(bound - 1).bit_length())
    for _ in range(passes):                               # k_reanchor_jump
        nxt = anc[anc]
        hop = hop + hop[anc]
        if np.array_equal(nxt, anc):
            break                                         # every chain has arrived: later passes add hop 0
        anc = nxt
    short = anc[anc] != anc                               # k_reanchor_hist
    if "short-flag-first-sweep" in wrong:
        short[SWEEP:] = False
    if "short-flag-lost" in wrong:
        short[:] = False
    depths = min(R, (1 << passes) + 1)
    assert depths == rc.hist_depths(R, c.bound) and (short.any() or hop.max() < depths)
    if short.any():
        return REFUSED
    count = np.bincount(hop, minlength=depths)
    if ("lds-counts-not-flushed" in wrong and depths <= rc.LDS_DEPTHS) or ("global-counts-lost" in wrong and depths > rc.LDS_DEPTHS):
        count[:] = 0
    if "last-lds-depth-dropped" in wrong and depths <= rc.LDS_DEPTHS:
        count[depths - 1] = 0
    if "lds-at-2049" in wrong and depths == rc.LDS_DEPTHS + 1:
        count[rc.LDS_DEPTHS] = 0
    off = np.concatenate([[0], np.cumsum(count)])         # k_reanchor_offsets
    levels = int(np.flatnonzero(count)[-1]) + 1 if count.any() else 0
    if off[levels] != R:
        return {"error": "the level offsets do not cover the rows"}
    return hop, off, levels


def _reanchor_run(c, plan, wrong=()):
    from oracle.pyoracle import replay
    hop, off, levels = plan
    R = len(c.parent)
    cfg = planner_config(**c.params)
    boxes = np.ascontiguousarray(c.boxes, np.float32).reshape(-1, 4)
    order = np.argsort(hop, kind="stable")                # k_reanchor_scatter: any order inside a level
    out = np.zeros((R, 4), np.float32)
    alive = np.zeros(R, bool)
    status = np.full(R, UNWRITTEN, np.uint8)
    for lv in range(levels):                              # k_reanchor_level, one launch a level
        rows = order[off[lv]:off[lv + 1]]
        if "level-past-sweep-dropped" in wrong:
            rows = rows[:SWEEP]
        if lv == 0:
            out[rows], status[rows] = c.state[rows], ORPHAN
            out[0], alive[0], status[0] = np.asarray(c.s0, np.float32)[:4], True, FREE
            continue
        par = c.parent[rows]
        live = alive[par]
        cut, run = rows[~live], rows[live]
        out[cut], status[cut] = c.state[cut], FREE | CUT
        if len(run):
            end, valid = replay(cfg, boxes, np.ascontiguousarray(out[c.parent[run]]), np.ascontiguousarray(c.ctrl[run, :3]),
                                threads=8)
            valid = np.asarray(valid, bool)
            out[run] = np.where(valid[:, None], end, c.state[run])
            alive[run] = valid
            status[run] = np.where(valid, FREE, BLOCKED)
    return {"state": out, "alive": alive, "status": status, "summary": summary_of(status, levels)}


def _same_plan(a, b) -> bool:
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and a == b
    return a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def _reanchor_true(name):
    c = R_BUILD[name]()
    plan = _reanchor_plan(c)
    return plan, (plan if isinstance(plan, dict) else _reanchor_run(c, plan))


def reanchor(name, wrong=()):
    c = R_BUILD[name]()
    true_plan, true_answer = _reanchor_true(name)
    if not wrong:
        return true_answer
    plan = _reanchor_plan(c, wrong)
    if isinstance(plan, dict):
        return plan
    if _same_plan(plan, true_plan) and "level-past-sweep-dropped" not in wrong:
        return true_answer                                # the same launches over the same rows
    return _reanchor_run(c, plan, wrong)


def _reanchor_same(name, got) -> bool:
    c = R_BUILD[name]()
    if c.refused or "refused" in got or "error" in got:
        return c.refused and got == REFUSED
    wout, walive, wstatus, wsum = c.model
    return got["summary"] == wsum and _same_arrays(got["status"], wstatus) and _same_arrays(got["alive"], walive) \
        and _same_arrays(got["state"], wout)


@pytest.mark.parametrize("name", R_CASES)
def test_reanchor_the_true_pass_is_the_model(name):
    assert _reanchor_same(name, reanchor(name)), name


@pytest.fixture(scope="module")
def r_table():
    return _table(R_CASES, R_WRONG, lambda n, w: not _reanchor_same(n, reanchor(n, (w,))))


@pytest.mark.parametrize("w", R_WRONG)
def test_reanchor_wrong_pass_is_caught(w, r_table):
    _check_wrong(w, r_table, R_CASES, R_CAUGHT_BY)


def test_reanchor_every_wrong_pass_is_caught_and_no_case_is_idle(r_table):
    _check_table(r_table, R_CASES, R_WRONG, R_CAUGHT_BY)
    assert set(R_CASES) <= set(rc.CASE_IDS)
    # the wrong passes whose kernels would throw, and the one that answers where it must refuse
    assert "error" in reanchor("chain-2047", ("last-lds-depth-dropped",)) and "error" in reanchor("chain-2048", ("lds-at-2049",))
    assert "summary" in reanchor("short-bound-past-sweep-4", ("short-flag-first-sweep",))
    assert reanchor("chain-2047-bound-1024") == REFUSED


# ================================================================ resample
S_WRONG = ("past-sweep-dropped", "request-0-past-sweep")


@functools.lru_cache(maxsize=None)
def _resample_want():
    case, nodes, period = sc.many_requests()
    return resample_model(case.state, case.ctrl, case.parent, nodes, period, **sc.params_of(case))


def resample(wrong=()) -> dict:
    """counts, status, offsets, edges and times by the kernels' own steps; `src`: the sample of the
    model a state is taken from (the sample's request and number m fix it), -1 for none."""
    case, nodes, period = sc.many_requests()
    R = len(case.parent)
    par = case.parent.tolist()
    chains, clocks, counts, status = [], [], [], []
    for node in nodes.tolist():                           # k_path_walk and k_resample_clock
        st, chain = path_of(par, node, R)
        T = clock_of(case.ctrl, chain) if st == OK else []
        status.append(st), chains.append(np.array(chain if st == OK else [], np.int64)), clocks.append(np.array(T))
        counts.append(count_of(T[-1], period) if st == OK else 0)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(offsets[-1])
    s = np.arange(total, dtype=np.int64)                  # k_path_resample, one lane a sample
    i = np.searchsorted(offsets[:len(nodes)], s, side="right") - 1     # the last request whose offset is <= s
    written = np.ones(total, bool)
    if "past-sweep-dropped" in wrong:
        written[SWEEP:] = False
    if "request-0-past-sweep" in wrong:
        i[SWEEP:] = 0
    m = s - offsets[i]
    edges, times, src = np.zeros(total, np.int32), np.zeros(total, np.float64), np.full(total, -1, np.int64)
    for q in np.unique(i[written]):
        mine = np.flatnonzero(written & (i == q))
        L, T, n = len(chains[q]), clocks[q], counts[q]
        if L == 0:
            continue                                      # no path to read: nothing the kernel could write rightly
        t = m[mine] * period
        k = np.where(m[mine] == n - 1, L, np.searchsorted(T, t, side="right"))
        end = k >= L
        edges[mine] = chains[q][np.where(end, L - 1, np.minimum(k, L - 1))]
        times[mine] = np.where(end, T[-1], t)
        src[mine] = np.where(m[mine] < n, offsets[q] + np.minimum(m[mine], n - 1), offsets[q] + n - 1)
    return {"counts": np.array(counts, np.int32), "status": np.array(status, np.uint8), "offsets": offsets, "edges": edges,
            "times": times, "src": src}


def _resample_same(got) -> bool:
    want = _resample_want()
    states = np.where((got["src"] >= 0)[:, None], want["states"][np.maximum(got["src"], 0)], np.float32(0))
    return all(_same_arrays(got[k], want[k]) for k in ("counts", "status", "offsets", "edges", "times")) \
        and _same_arrays(states, want["states"])


def test_resample_the_true_pass_is_the_model():
    got = resample()
    assert _same_arrays(got["src"], np.arange(len(got["src"]), dtype=np.int64)) and _resample_same(got)


@pytest.mark.parametrize("w", S_WRONG)
def test_resample_wrong_pass_is_caught(w):
    got = resample((w,))
    assert not _resample_same(got), w
    assert (got["src"][:SWEEP] == np.arange(SWEEP)).all()          # caught by the samples past the sweep alone

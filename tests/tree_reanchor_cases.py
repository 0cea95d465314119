"""The trees, root states and box lists of the re-anchoring tests (tests/test_tree_reanchor.py on
the host twin, tests/test_gpu_tree_reanchor.py on the kernels), built on the re-check's table
(tests/tree_recheck_cases.py), each with the model's answer (tests/tree_reanchor_model.py),
computed once per process.  A case is an RCase: a tree, its boxes, the plan's parameters, the
new root state s0 and a depth bound.

  grown trees   every GROWN tree against its own boxes with s0 = the stored root bits (same),
                one ulp off in x (ulp) and displaced by a tracking error (moved)
  chain-*       single chains of CHAIN_DEPTHS edges: every row is a level of its own
  star, level-* one level of many rows; level sizes either side of 64 and 256
  rows-*        ROW_COUNTS
  far-parent    random parents behind a chain: a deep row's parent is a far lower row, so the
                depth does not follow the row order
  parent-*      crafted parents on rows 1, 5, the last and the busiest: their descendants are cut
  blocked, wall a box on the busiest row's REPLAYED end point; the workspace narrowed
  boxes-*       BOX_COUNTS, either side of every obstacle form's threshold; NaN boxes
  bound-*       depthBound 0, exact, no power of two, and too small (refused)
  star-sweep+77, recursive-sweep+77   SWEEP + 77 rows (SWEEP = 524,288, one sweep of the grid): one level
                of more than a sweep of rows; a random recursive tree of 33 levels with depthBound 0
                (global depth counters, depths = rows) and 64 (65 LDS counters)
  short-bound-past-sweep   only rows of the last sweep lie deeper than the bound covers (refused)
  rows-2047 .. 2049, chain-2046 .. 2048   2,047 and 2,048 depth counters (LDS) and 2,049 (global);
                chains that put a row on the last counter of each

Plain numpy plus the CPU oracle at call time; no GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import tree_recheck_cases as tc
from edge_scenarios import up
from scenarios import demo_boxes, demo_plus
from tree_query_cases import SWEEP
from tree_recheck_model import depths, replay_rows
from tree_reanchor_model import reanchor_model

# A tracking error: a few centimetres and a few hundredths of a radian (x, y, theta, v).
MOVED = (0.05, -0.03, 0.02, 0.0)
S0_KINDS = ("same", "ulp", "moved")
LEVEL_SIZES = (63, 64, 65, 255, 256, 257)
STAR_ROWS = 1000


@dataclass(frozen=True, eq=False)
class RCase:
    name: str
    state: np.ndarray
    ctrl: np.ndarray
    parent: np.ndarray
    boxes: np.ndarray
    params: dict                 # numDisc, agentLength, width, height, agent
    s0: np.ndarray
    bound: int = 0
    refused: bool = False        # the bound is below the longest chain: the device refuses the call

    @functools.cached_property
    def model(self):
        return reanchor_model(self.state, self.ctrl, self.parent, self.s0, self.boxes, **self.params)


def new_root(case, kind) -> np.ndarray:
    root = case.state[0].copy()
    if kind == "ulp":
        root[0] = up(root[0])
    elif kind == "moved":
        root = (root + np.asarray(MOVED, np.float32)).astype(np.float32)
    return root


def of(case, kind="moved", name=None, **kw) -> RCase:
    return RCase(name or f"{case.name}-{kind}", case.state, case.ctrl, case.parent, case.boxes, case.params,
                 new_root(case, kind), **kw)


@functools.lru_cache(maxsize=None)
def grown(agent, L, D, kind) -> RCase:
    return of(tc.grown(agent, L, D), kind)


@functools.lru_cache(maxsize=None)
def chain(depth, where, kind="moved", bound=0, refused=False) -> RCase:
    c = tc.chain_case(depth, where)
    name = f"{c.name}-{kind}" + (f"-bound-{bound}" if bound else "")
    return of(c, kind, name, bound=bound, refused=refused)


@functools.lru_cache(maxsize=None)
def star(rows) -> RCase:
    return of(tc.star_case(rows))


@functools.lru_cache(maxsize=None)
def rows_case(rows) -> RCase:
    return of(tc.rows_case(rows))


@functools.lru_cache(maxsize=None)
def far_parent() -> RCase:
    """A chain of 40 rows, then 660 rows whose parent is any lower row: short edges (at most 0.3 s)
    from the middle of the workspace, whose wall stands half a metre from the root; the stored
    states are anything inside it."""
    rng = np.random.default_rng(40)
    R, head = 700, 40
    parent = np.empty(R, np.int32)
    parent[:head] = np.arange(-1, head - 1)
    parent[head:] = [rng.integers(0, r) for r in range(head, R)]
    parent[R - 1] = 1                                   # the last row hangs on row 1
    state = rng.uniform(1.0, 19.0, (R, 4)).astype(np.float32)
    state[0] = (10.0, 10.0, 0.3, 0.5)
    ctrl = np.zeros((R, 4), np.float32)
    ctrl[1:, 0] = rng.uniform(-5.0, 5.0, R - 1)
    ctrl[1:, 1] = rng.uniform(-3.1, 3.1, R - 1)
    ctrl[1:, 2] = rng.uniform(0.06, 0.3, R - 1)
    d = depths(parent)
    assert d[R - 1] == 2 and d[R - 2] != 2 and (np.diff(d[head:]) < 0).any() and d.max() >= head - 1
    return RCase("far-parent", state, ctrl, parent, demo_boxes(), dict(tc.CHAIN_PARAMS, width=10.5), state[0].copy())


@functools.lru_cache(maxsize=None)
def parent_case(kind) -> RCase:
    return of(tc.parent_case(kind))


@functools.lru_cache(maxsize=None)
def blocked() -> RCase:
    """One box on the end point the busiest row has AFTER the re-anchoring (not on its stored one)."""
    base = grown(*tc.MAIN, "moved")
    r = tc.busiest_row(*tc.MAIN)
    out, alive, _, _ = base.model
    assert alive[r]
    x, y = out[r, :2]
    return RCase("blocked-replayed", base.state, base.ctrl, base.parent, demo_plus((x - 0.02, y - 0.02, x + 0.02, y + 0.02)),
                 base.params, base.s0)


@functools.lru_cache(maxsize=None)
def wall() -> RCase:
    base = grown(*tc.MAIN, "moved")
    return RCase("wall", base.state, base.ctrl, base.parent, base.boxes, dict(base.params, width=14.0), base.s0)


@functools.lru_cache(maxsize=None)
def boxes_case(count) -> RCase:
    return of(tc.boxes_case(count))


@functools.lru_cache(maxsize=None)
def nan_case(count) -> RCase:
    return of(tc.nan_case(count))


@functools.lru_cache(maxsize=None)
def bound_case(which) -> RCase:
    """Bounds count the rows of the longest chain.  A chain of 9 rows: 0 (rows), 9 (exact), 11 (no
    power of two), 4 (two passes cover four edges of eight: refused).  The main grown tree with the
    bound its planner would give (13 rows: 12 iterations and the root).  A chain of 257 rows with
    257 (exact) and 100 (seven passes cover 128 edges of 256: refused)."""
    if which == "grown-13":
        g = grown(*tc.MAIN, "moved")
        assert int(depths(g.parent).max()) + 1 <= 13
        return RCase("bound-grown-13", g.state, g.ctrl, g.parent, g.boxes, g.params, g.s0, bound=13)
    depth, bound = {"0": (8, 0), "exact": (8, 9), "odd": (8, 11), "short": (8, 4), "exact-257": (256, 257),
                    "short-257": (256, 100)}[which]
    return chain(depth, "last", "moved", bound, which.startswith("short"))


BOUND_KINDS = ("0", "exact", "odd", "short", "exact-257", "short-257", "grown-13")


# ---------------------------------------------------------------- past one grid sweep, and the LDS seam
def big_star() -> RCase:
    return star(SWEEP + 77)


@functools.lru_cache(maxsize=None)
def _recursive_tree():
    """SWEEP + 77 rows, row r the child of a uniformly drawn lower row (a random recursive tree,
    about 2 ln rows levels), with far_parent()'s root and controls."""
    rng = np.random.default_rng(1)
    R = SWEEP + 77
    r = np.arange(R, dtype=np.int64)
    parent = np.minimum(np.floor(rng.random(R) * r).astype(np.int64), r - 1).astype(np.int32)
    parent[0] = -1
    state = rng.uniform(1.0, 19.0, (R, 4)).astype(np.float32)
    state[0] = (10.0, 10.0, 0.3, 0.5)
    ctrl = np.zeros((R, 4), np.float32)
    ctrl[1:, 0] = rng.uniform(-5.0, 5.0, R - 1)
    ctrl[1:, 1] = rng.uniform(-3.1, 3.1, R - 1)
    ctrl[1:, 2] = rng.uniform(0.06, 0.3, R - 1)
    for a in (state, ctrl, parent):
        a.setflags(write=False)
    return state, ctrl, parent


@functools.lru_cache(maxsize=None)
def recursive(bound=0) -> RCase:
    """bound 0: depths = rows, global depth counters and 2,049 rounds of k_reanchor_offsets; bound
    64: 6 passes, 65 depths, LDS counters over every sweep."""
    state, ctrl, parent = _recursive_tree()
    return RCase(f"recursive-sweep+77-bound-{bound}", state, ctrl, parent, demo_boxes(), tc.CHAIN_PARAMS,
                 state[0].copy(), bound=bound)


SHORT_STAR, SHORT_CHAIN = SWEEP + 68, 9


@functools.lru_cache(maxsize=None)
def short_bound_past_sweep(bound) -> RCase:
    """A star of SWEEP + 68 rows and, behind it, a chain of 9 rows hanging on row 0: only rows of
    the last sweep lie more than 4 edges deep.  bound 4 (two passes cover four edges) is refused."""
    c = tc.star_case(SHORT_STAR + SHORT_CHAIN)
    parent = c.parent.copy()
    parent[SHORT_STAR + 1:] = np.arange(SHORT_STAR, SHORT_STAR + SHORT_CHAIN - 1)
    ctrl = c.ctrl.copy()
    ctrl[SHORT_STAR:, 2] = 0.07                          # short edges: the chain stays near the root
    assert parent[SHORT_STAR] == 0 and not parent[1:SHORT_STAR].any() and len(parent) == SWEEP + 77
    return of(c.with_("short-bound-past-sweep", parent=parent, ctrl=ctrl), "moved", f"short-bound-past-sweep-{bound}",
              bound=bound, refused=bound == 4)


LONG_CHAIN_ROWS = 2050


@functools.lru_cache(maxsize=None)
def _long_chain():
    """2,050 rows, row r the child of row r - 1, every one the model's own replay without boxes: the
    car circles inside [6.7, 13.3] x [5.99, 12.5] (steering 0.3, 0.07 s an edge, a = +1 / -1 in turn)."""
    n = LONG_CHAIN_ROWS
    state = np.zeros((n, 4), np.float32)
    ctrl = np.zeros((n, 4), np.float32)
    state[0] = (10.0, 6.0, 0.0, 1.0)
    ctrl[1:, 0] = np.where(np.arange(1, n) % 2 == 1, 1.0, -1.0)
    ctrl[1:, 1] = 0.3
    ctrl[1:, 2] = 0.07
    none = np.zeros((0, 4), np.float32)
    for r in range(1, n):
        _, out, valid = replay_rows(np.stack([state[r - 1], state[r - 1]]), ctrl[[r, r]], [-1, 0], none, threads=1,
                                    **tc.CHAIN_PARAMS)
        assert valid[1], r
        state[r] = out[1]
        ctrl[r, 3] = ctrl[r - 1, 3] + ctrl[r, 2]
    x, y = state[:, 0], state[:, 1]
    assert 6.7 <= x.min() and x.max() <= 13.3 and 5.99 <= y.min() and y.max() <= 12.5
    assert np.hypot(np.diff(x.astype(np.float64)), np.diff(y.astype(np.float64))).min() >= 0.05
    return state, ctrl, np.arange(-1, n - 1, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def long_chain(edges, bound=0, refused=False) -> RCase:
    """`edges` + 1 rows of _long_chain(), every row a level of its own, s0 displaced by MOVED."""
    state, ctrl, parent = _long_chain()
    rows = edges + 1
    c = tc.Case(f"chain-{edges}", state[:rows].copy(), ctrl[:rows].copy(), parent[:rows].copy(),
                np.zeros((0, 4), np.float32), tc.CHAIN_PARAMS)
    return of(c, "moved", f"chain-{edges}" + (f"-bound-{bound}" if bound else ""), bound=bound, refused=refused)


@functools.lru_cache(maxsize=None)
def seam_rows(rows, bound=0) -> RCase:
    """The first `rows` rows of the main grown tree (two levels): 2,047 and 2,048 rows give as many
    depth counters, in LDS; 2,049 rows, also with bound 2,048 (11 passes), give 2,049, global ones."""
    return of(tc.rows_case(rows), "moved", f"rows-{rows}" + (f"-bound-{bound}" if bound else ""), bound=bound)


LDS_DEPTHS = 2048                    # kReanchorLdsDepths: the depth counters k_reanchor_hist keeps in LDS
SEAM_ROWS = (2047, 2048, 2049)
LONG_CHAIN_EDGES = (2046, 2047, 2048)


def hist_depths(rows, bound=0) -> int:
    """The depth counters a call allocates: min(rows, 2^passes + 1), passes = ceil(log2(the bound))."""
    b = min(bound, rows) if bound > 0 else rows
    passes = max(1, int(b - 1).bit_length())
    return min(rows, (1 << passes) + 1)


def past_sweep_cases() -> list:
    out = [("star-sweep+77", big_star), ("recursive-sweep+77", functools.partial(recursive, 0)),
           ("recursive-sweep+77-bound-64", functools.partial(recursive, 64)),
           ("short-bound-past-sweep-4", functools.partial(short_bound_past_sweep, 4)),
           ("short-bound-past-sweep-9", functools.partial(short_bound_past_sweep, 9))]
    out += [(f"rows-{n}", functools.partial(seam_rows, n)) for n in SEAM_ROWS]
    out.append(("rows-2049-bound-2048", functools.partial(seam_rows, 2049, 2048)))
    out += [(f"chain-{e}", functools.partial(long_chain, e)) for e in LONG_CHAIN_EDGES]
    out += [("chain-2047-bound-1025", functools.partial(long_chain, 2047, 1025)),
            ("chain-2047-bound-1024", functools.partial(long_chain, 2047, 1024, True))]
    return out


def cases() -> list:
    """(id, builder) of every case the host twin and the kernels are held to the model on."""
    out = []
    for g, gid in zip(tc.GROWN, tc.GROWN_IDS):
        out += [(f"{gid}-{k}", functools.partial(grown, *g, k)) for k in S0_KINDS]
    out += [(f"chain-{d}-last", functools.partial(chain, d, "last")) for d in tc.CHAIN_DEPTHS]
    out += [(f"chain-{d}-first", functools.partial(chain, d, "first", "same")) for d in (1, 9, 257)]
    out += [(f"chain-{d}-same", functools.partial(chain, d, "last", "same")) for d in (8, 257)]
    out.append((f"star-{STAR_ROWS}", functools.partial(star, STAR_ROWS)))
    out += [(f"level-{n}", functools.partial(star, n + 1)) for n in LEVEL_SIZES]
    out += [(f"rows-{n}", functools.partial(rows_case, n)) for n in tc.ROW_COUNTS]
    out.append(("far-parent", far_parent))
    out += [(f"parent-{k}", functools.partial(parent_case, k)) for k in tc.PARENT_KINDS]
    out += [("blocked-replayed", blocked), ("wall", wall)]
    out += [(f"boxes-{n}", functools.partial(boxes_case, n)) for n in tc.BOX_COUNTS]
    out += [(f"boxes-nan-{n}", functools.partial(nan_case, n)) for n in (5, 600)]
    out += [(f"bound-{k}", functools.partial(bound_case, k)) for k in BOUND_KINDS]
    out += past_sweep_cases()
    return out


CASES = cases()
CASE_IDS = [i for i, _ in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)

BAD_ROOTS = {"nan-x": (np.nan, 5.0, 0.0, 0.0), "nan-v": (5.0, 5.0, 0.0, np.nan), "inf-y": (5.0, np.inf, 0.0, 0.0),
             "minus-inf-theta": (5.0, 5.0, -np.inf, 0.0)}

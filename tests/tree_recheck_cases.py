"""The trees and box lists of the re-check tests (tests/test_tree_recheck.py on the host twin,
tests/test_gpu_tree_recheck.py on the kernels), each with the model's answer
(tests/tree_recheck_model.py).  A case is a Case: state, ctrl, parent, boxes, the plan's
parameters, and the model's (status, summary, alive), computed once per process.

  grown trees   the CPU oracle's tree of the small base of tests/scenarios.py (16,384 slots, 12
                iterations, complete clear), car and point, L = 1 and 1.3, numDisc 1, 10, 13
  own           against the plan's own boxes
  blocked       one box on the stored end point of the row of depth >= 2 with most descendants
  edge-*        a box edge, or a wall, on a row's own float, one ulp towards it, one ulp away
                (the technique of tests/edge_scenarios.py)
  parent-*      crafted parents on rows 1, 5 and the last, and on the row with most descendants
  stale-*       one stored state moved by one ulp
  d6            the reference-clear tree of tests/goal_scenarios.py (rows counted, never written)
  chain-*       single chains built from the model's own replays
  boxes-*       box counts either side of every obstacle form's threshold; NaN boxes
  rows-*, star  row counts round the wave and workgroup sizes; a star of `rows` rows

Plain numpy plus the CPU oracle at call time; no GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from edge_scenarios import down, up
from scenarios import Scenario, demo_boxes, demo_plus, demo_prefix, make_oracle, random_boxes
from tree_recheck_model import BLOCKED, FREE, depths, descendants, recheck_model, replay_rows, tree_arrays

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
GROWN = [(agent, L, D) for agent, L in (("car", 1.0), ("car", 1.3), ("point", 1.0)) for D in (1, 10, 13)]
GROWN_IDS = [f"{a}-L{L:g}-D{D}" for a, L, D in GROWN]
MAIN = ("car", 1.0, 10)          # the tree the crafted cases start from
CHAIN_DEPTHS = (1, 2, 3, 4, 5, 8, 9, 255, 256, 257)
BOX_COUNTS = (0, 1, 8, 9, 600, 2048, 2049, 3000)
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)
SMALL = 16385                    # rows of the prefix the long box lists run on


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    state: np.ndarray
    ctrl: np.ndarray
    parent: np.ndarray
    boxes: np.ndarray
    params: dict                 # numDisc, agentLength, width, height, agent

    @functools.cached_property
    def model(self):
        return recheck_model(self.state, self.ctrl, self.parent, self.boxes, **self.params)

    def with_(self, name, **changes):
        f = dict(name=name, state=self.state, ctrl=self.ctrl, parent=self.parent, boxes=self.boxes, params=self.params)
        f.update(changes)
        return Case(**f)

    def prefix(self, rows, name=None):
        return self.with_(name or f"{self.name}-rows-{rows}", state=self.state[:rows].copy(), ctrl=self.ctrl[:rows].copy(),
                          parent=self.parent[:rows].copy())


@functools.lru_cache(maxsize=None)
def grown(agent, L, D) -> Case:
    sc = Scenario(name=f"recheck-{agent}-L{L:g}-D{D}", family="recheck", targets="a grown tree",
                  kw=dict(agent=agent, agentLength=L, numDisc=D), boxes=demo_boxes)
    o = make_oracle(sc)
    s, p, c = o.tree()
    state, ctrl, parent = tree_arrays(s, p, c, o.info()["treeSize"])
    cfg, _ = sc.config()
    params = dict(numDisc=D, agentLength=L, width=cfg["width"], height=cfg["height"], agent=agent)
    return Case(f"{agent}-L{L:g}-D{D}-own", state, ctrl, parent, demo_boxes(), params)


@functools.lru_cache(maxsize=None)
def busiest_row(agent, L, D) -> int:
    """The row of depth >= 2 with the most descendants (the lowest such row)."""
    c = grown(agent, L, D)
    n = descendants(c.parent)
    n[depths(c.parent) < 2] = -1
    r = int(np.argmax(n))
    assert n[r] > 0, "no row of depth >= 2 has a descendant"
    return r


@functools.lru_cache(maxsize=None)
def blocked(agent, L, D) -> Case:
    c = grown(agent, L, D)
    x, y = c.state[busiest_row(agent, L, D), :2]
    return c.with_(c.name.replace("-own", "-blocked"), boxes=demo_plus((x - 0.05, y - 0.05, x + 0.05, y + 0.05)))


# ---------------------------------------------------------------- verdict edges
def _slab(axis, edge, W, H):
    """A box over the whole workspace beyond `edge` on one axis."""
    return (edge, -1.0, W + 1.0, H + 1.0) if axis == 0 else (-1.0, edge, W + 1.0, H + 1.0)


@functools.lru_cache(maxsize=None)
def edge_row(agent, L, D, axis) -> int:
    """A row whose stored coordinate on `axis` is the box edge of the edge cases: of the rows
    furthest out, the first that the model calls FREE with the edge on its float or one ulp
    beyond, and BLOCKED with the edge one ulp nearer (its last step ends on its largest
    coordinate, and no other step of its reaches as far)."""
    c = grown(agent, L, D)
    W, H = c.params["width"], c.params["height"]
    for r in np.argsort(-c.state[:, axis], kind="stable")[:64]:
        r = int(r)
        if r == 0:
            continue
        v = c.state[r, axis]
        got = []
        for edge in (v, down(v), up(v)):
            one = c.prefix(r + 1).with_("probe", boxes=np.array([_slab(axis, edge, W, H)], np.float32))
            got.append(int(one.model[0][r]))
        if got == [FREE, BLOCKED, FREE]:
            return r
    raise AssertionError("no row puts the three verdicts on one float")


@functools.lru_cache(maxsize=None)
def edge_case(agent, L, D, axis, kind, variant) -> Case:
    """kind 'box': the slab's near edge; 'wall': width (axis 0) or height (axis 1)."""
    c = grown(agent, L, D)
    r = edge_row(agent, L, D, axis)
    v = c.state[r, axis]
    name = f"{agent}-L{L:g}-D{D}-edge-{kind}-{'xy'[axis]}-{variant}"
    if kind == "box":
        edge = {"at": v, "in": down(v), "out": up(v)}[variant]
        return c.with_(name, boxes=demo_plus(_slab(axis, edge, c.params["width"], c.params["height"])))
    wall = {"at": v, "in": up(v), "out": down(v)}[variant]     # `in`: the row stays inside
    key = "width" if axis == 0 else "height"
    return c.with_(name, params=dict(c.params, **{key: float(wall)}))


# ---------------------------------------------------------------- crafted parents, stale states
PARENT_KINDS = ("minus1", "self", "next", "int_min", "int_max")


def parent_rows() -> tuple:
    """Rows 1, 5 and the last, and the busiest row: rows 1 and 5 of this tree have no descendants."""
    return (1, 5, busiest_row(*MAIN), len(grown(*MAIN).parent) - 1)


@functools.lru_cache(maxsize=None)
def parent_case(kind) -> Case:
    c = grown(*MAIN)
    R = len(c.parent)
    p = c.parent.copy()
    for r in parent_rows():
        p[r] = {"minus1": -1, "self": r, "next": r + 1, "int_min": INT_MIN, "int_max": INT_MAX}[kind]
    return c.with_(f"parent-{kind}", parent=p)


@functools.lru_cache(maxsize=None)
def stale_case(column) -> Case:
    """column 0: x, 2: theta of the busiest row, one ulp up."""
    c = grown(*MAIN)
    s = c.state.copy()
    r = busiest_row(*MAIN)
    s[r, column] = up(s[r, column])
    return c.with_(f"stale-{ {0: 'x', 2: 'theta'}[column]}", state=s)


@functools.lru_cache(maxsize=None)
def d6_case() -> Case:
    """The reference's partial GNew clear at M = 1000 (tests/goal_scenarios.py, D6-partial-clear)."""
    import goal_scenarios as gs
    sc = gs.scenario(gs.D6_PARTIAL, (2.0, 18.0), 0.0)
    o = make_oracle(sc)
    s, p, c = o.tree()
    state, ctrl, parent = tree_arrays(s, p, c, o.info()["treeSize"])
    cfg, extra = sc.config()
    params = dict(numDisc=cfg["numDisc"], agentLength=cfg["agentLength"], width=cfg["width"], height=cfg["height"],
                  agent=extra.get("agent", "car"))
    return Case("d6", state, ctrl, parent, sc.obstacles(), params)


# ---------------------------------------------------------------- chains
CHAIN_PARAMS = dict(numDisc=10, agentLength=1.0, width=20.0, height=20.0, agent="car")


@functools.lru_cache(maxsize=None)
def _chain():
    """258 rows, row r the child of row r - 1, every one the model's own replay (no boxes): x
    grows by about 0.07 per row from 1.0, the heading turns slowly."""
    n = max(CHAIN_DEPTHS) + 1
    state = np.zeros((n, 4), np.float32)
    ctrl = np.zeros((n, 4), np.float32)
    state[0] = (1.0, 5.0, 0.0, 1.0)
    ctrl[1:, 0] = np.where(np.arange(1, n) % 2 == 1, 1.0, -1.0)
    ctrl[1:, 1] = 0.05
    ctrl[1:, 2] = 0.07
    none = np.zeros((0, 4), np.float32)
    for r in range(1, n):
        _, out, valid = replay_rows(np.stack([state[r - 1], state[r - 1]]), ctrl[[r, r]], [-1, 0], none, threads=1,
                                    **CHAIN_PARAMS)
        assert valid[1]
        state[r] = out[1]
        ctrl[r, 3] = ctrl[r - 1, 3] + ctrl[r, 2]
    assert np.all(np.diff(state[:, 0]) > 0.03)   # x ascends: a slab between two rows meets one row's span
    return state, ctrl, np.arange(-1, n - 1, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def chain_case(depth, where) -> Case:
    """`depth` edges; where = 'first': a slab inside row 1's span, 'last': inside the last row's."""
    state, ctrl, parent = _chain()
    rows = depth + 1
    r = 1 if where == "first" else depth
    x0, x1 = state[r - 1, 0], state[r, 0]
    box = (x0 + 0.4 * (x1 - x0), -1.0, x0 + 0.6 * (x1 - x0), 21.0)   # strictly between the two rows' floats
    return Case(f"chain-{depth}-{where}", state[:rows].copy(), ctrl[:rows].copy(), parent[:rows].copy(),
                np.array([box], np.float32), CHAIN_PARAMS)


# ---------------------------------------------------------------- box lists, row counts, star
def box_list(count) -> np.ndarray:
    if count <= 8:
        return demo_prefix(count)
    return random_boxes(count, 20.0, 20.0, 7, 0.3 if count <= 2048 else 0.08, 0.8)


@functools.lru_cache(maxsize=None)
def boxes_case(count) -> Case:
    return grown(*MAIN).prefix(SMALL).with_(f"boxes-{count}", boxes=box_list(count))


@functools.lru_cache(maxsize=None)
def nan_case(count) -> Case:
    nan4 = (np.nan,) * 4
    boxes = demo_plus(nan4)[[0, 1, 5, 2, 3]] if count == 5 else random_boxes(600, 20.0, 20.0, 7, 0.3, 0.8, planted=nan4)
    assert len(boxes) == count and np.isnan(boxes).all(axis=1).sum() == 1
    return grown(*MAIN).prefix(SMALL).with_(f"boxes-nan-{count}", boxes=boxes)


@functools.lru_cache(maxsize=None)
def rows_case(rows) -> Case:
    return blocked(*MAIN).prefix(rows, f"rows-{rows}")


@functools.lru_cache(maxsize=None)
def star_case(rows) -> Case:
    """The root and rows - 1 children of it, each what the model's replay makes of seeded controls
    against the demo's boxes (a child that ends invalid is stored where its replay stopped)."""
    rng = np.random.default_rng(rows)
    state = np.zeros((rows, 4), np.float32)
    ctrl = np.zeros((rows, 4), np.float32)
    state[0] = (5.0, 5.0, 0.0, 0.0)
    ctrl[1:, 0] = rng.uniform(-5.0, 5.0, rows - 1)
    ctrl[1:, 1] = rng.uniform(-3.1, 3.1, rows - 1)
    ctrl[1:, 2] = rng.uniform(0.06, 1.05, rows - 1)
    ctrl[1:, 3] = ctrl[1:, 2]
    parent = np.zeros(rows, np.int32)
    parent[0] = -1
    _, out, _ = replay_rows(np.broadcast_to(state[0], (rows, 4)), ctrl, parent, demo_boxes(), **CHAIN_PARAMS)
    state[1:] = out[1:]
    return Case(f"star-{rows}", state, ctrl, parent, demo_boxes(), CHAIN_PARAMS)


def cpu_cases() -> list:
    """(id, builder) of every case both the host twin and the kernels are held to the model on."""
    out = []
    for g, gid in zip(GROWN, GROWN_IDS):
        out.append((f"{gid}-own", functools.partial(grown, *g)))
        out.append((f"{gid}-blocked", functools.partial(blocked, *g)))
    for g in (MAIN, ("point", 1.0, 10), ("car", 1.3, 13)):
        for axis in (0, 1):
            for kind in ("box", "wall"):
                for v in ("at", "in", "out"):
                    out.append((f"{g[0]}-L{g[1]:g}-D{g[2]}-edge-{kind}-{'xy'[axis]}-{v}",
                                functools.partial(edge_case, *g, axis, kind, v)))
    out += [(f"parent-{k}", functools.partial(parent_case, k)) for k in PARENT_KINDS]
    out += [("stale-x", functools.partial(stale_case, 0)), ("stale-theta", functools.partial(stale_case, 2))]
    out.append(("d6", d6_case))
    out += [(f"chain-{d}-{w}", functools.partial(chain_case, d, w)) for d in CHAIN_DEPTHS for w in ("first", "last")]
    out += [(f"boxes-{n}", functools.partial(boxes_case, n)) for n in BOX_COUNTS]
    out += [(f"boxes-nan-{n}", functools.partial(nan_case, n)) for n in (5, 600)]
    return out


CPU_CASES = cpu_cases()
CPU_IDS = [i for i, _ in CPU_CASES]
assert len(set(CPU_IDS)) == len(CPU_IDS)

"""The trees, masks and roots of the extraction tests (tests/test_tree_extract.py on the host
twin, tests/test_gpu_tree_extract.py on the kernels).  A case is an ExtractCase: a tree in the
planner's layout, a root and a keep mask (None: the NULL mask); the model's answer
(tests/tree_extract_model.py) is computed once per process.

  grown-*     the oracle-grown trees of tests/tree_recheck_cases.py (16,384 slots, 12 iterations)
  chain-*     single chains of 1, 2, 3, 64, 65, 257 rows
  star        a star of 257 rows
  rows-*      row counts round the wave and the workgroup; round the tile and one row more than a
              full round of the offsets workgroup, both read from sbmp_tree_extract_info; past one
              sweep of the row grid (SWEEP + 77 and 2 SWEEP + 1 rows: the later rounds of mark, jump
              and gather, three and five rounds of the offsets workgroup) and one row past one sweep
              of the tile grid (2,048 tiles + 1 row: the second round of count and number), that one
              also with every member but row 0 in the last 301 rows
  mask-*    NULL and all ones, all zero, the root only, alternating, bytes 2 and 0x80 as kept, a
              zero in the middle of a chain (its kept descendants are detached), a zero on the
              row with most descendants, every member packed into the last tile, every first
              lane of a wave and every last
  root-*      0, a leaf, R - 1, the row with most descendants, the D6 rows 993-999 of
              tests/goal_scenarios.py's reference-clear tree, a row that is masked, row SWEEP + 5
              of 2 SWEEP + 1 (`below` counts more than one sweep of rows)
  parent-*    the crafted parents of the re-check cases (-1, r, r + 1, INT_MIN, INT_MAX) on
              ordinary rows and on the root itself

The synthetic trees (rows-*, packed, lanes) hold random bit patterns as floats, NaNs included:
the extraction copies bytes and never reads a float but rootCost.  Plain numpy plus the CPU oracle
at call time; no GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import tree_recheck_cases as tc
from tree_extract_model import extract_model
from tree_query_cases import SWEEP
from tree_recheck_model import descendants

SWEEP_TILES = SWEEP // 256        # tiles of one sweep of k_extract_count / k_extract_number: a workgroup a tile
PAST_SWEEP = ("sweep+77", "2sweep+1", "tiles+1")
CHAIN_ROWS = (1, 2, 3, 64, 65, 257)
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)
D6_ROWS = tuple(range(993, 1000))


@dataclass(frozen=True, eq=False)
class ExtractCase:
    name: str
    state: np.ndarray
    ctrl: np.ndarray
    parent: np.ndarray
    root: int = 0
    keep: Optional[np.ndarray] = None

    @functools.cached_property
    def model(self):
        return extract_model(self.state, self.ctrl, self.parent, self.root, self.keep)

    @property
    def rows(self):
        return len(self.parent)


def of(tree, name, root=0, keep=None) -> ExtractCase:
    """A case over the arrays of a tests/tree_recheck_cases.py Case (or another ExtractCase)."""
    return ExtractCase(name, tree.state, tree.ctrl, tree.parent, int(root), keep)


@functools.lru_cache(maxsize=None)
def layout():
    """tileRows and the rows of one full round of the offsets workgroup, from the library."""
    from cudasbmp_amd import tree_extract_info
    i = tree_extract_info(0)
    return i["tileRows"], i["tileRows"] * i["roundTiles"]


def past_sweep_rows(what) -> int:
    """Row counts past one sweep of the row grid (SWEEP rows: mark, jump, gather) and one row past
    one sweep of the tile grid (SWEEP_TILES tiles: count, number)."""
    tile, _ = layout()
    return {"sweep+77": SWEEP + 77, "2sweep+1": 2 * SWEEP + 1, "tiles+1": SWEEP_TILES * tile + 1}[what]


@functools.lru_cache(maxsize=None)
def synthetic(rows, seed=0, hub=None, packed_from=None) -> ExtractCase:
    """`rows` rows of random bits.  Parents: a random lower row (a random recursive tree, depth about
    ln rows); hub: every row above `hub` hangs on it, the rows below it are orphans; packed_from:
    the rows from there on pick their parent among themselves."""
    rng = np.random.default_rng(1000 + seed)
    state = rng.integers(0, 2 ** 32, (rows, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    ctrl = rng.integers(0, 2 ** 32, (rows, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = np.arange(rows, dtype=np.int64)
    if hub is not None:
        parent = np.where(r > hub, hub, -1)
    else:
        lo = np.zeros(rows, np.int64) if packed_from is None else np.where(r > packed_from, packed_from, 0)
        parent = lo + (rng.random(rows) * (r - lo)).astype(np.int64)
        parent = np.minimum(parent, r - 1)
        parent[0] = -1
    return ExtractCase(f"synthetic-{rows}", state, ctrl, parent.astype(np.int32))


def main_tree():
    return tc.grown(*tc.MAIN)


def chain(rows) -> ExtractCase:
    state, ctrl, parent = tc._chain()
    return ExtractCase(f"chain-{rows}", state[:rows].copy(), ctrl[:rows].copy(), parent[:rows].copy())


@functools.lru_cache(maxsize=None)
def a_leaf() -> int:
    """The lowest row of the main tree above row 0 that is nobody's parent."""
    t = main_tree()
    n = descendants(t.parent)
    return int(np.flatnonzero(n[1:] == 0)[0]) + 1


def _mask(rows, fn):
    return fn(np.arange(rows)).astype(np.uint8)


def masks_for(tree, busiest) -> list:
    """(suffix, keep) over one tree with root 0."""
    R = len(tree.parent)
    rng = np.random.default_rng(R)
    only_root = np.zeros(R, np.uint8)
    only_root[0] = 1
    odd_bytes = rng.choice(np.array([0, 2, 0x80], np.uint8), R)
    odd_bytes[0] = 0x80
    no_busiest = np.ones(R, np.uint8)
    no_busiest[busiest] = 0
    return [("null", None), ("ones", np.ones(R, np.uint8)), ("zero", np.zeros(R, np.uint8)), ("root-only", only_root),
            ("alternating", _mask(R, lambda r: r % 2 == 0)), ("bytes-2-0x80", odd_bytes), ("no-busiest", no_busiest)]


def all_cases() -> list:
    """(id, builder) of every case both the host twin and the kernels are held to the model on."""
    out = []

    def add(name, fn):
        out.append((name, fn))

    for g, gid in zip(tc.GROWN, tc.GROWN_IDS):
        add(f"grown-{gid}", functools.partial(lambda g, gid: of(tc.grown(*g), f"grown-{gid}"), g, gid))
    for n in CHAIN_ROWS:
        add(f"chain-{n}", functools.partial(chain, n))
        if n > 1:
            add(f"chain-{n}-from-last", functools.partial(lambda n: of(chain(n), f"chain-{n}-from-last", n - 1), n))
    add("star", lambda: of(tc.star_case(257), "star"))
    for n in ROW_COUNTS:
        add(f"rows-{n}", functools.partial(lambda n: of(tc.rows_case(n), f"rows-{n}"), n))

    def seam(n, masked):
        c = synthetic(n, seed=n % 97)
        keep = (np.random.default_rng(n).random(n) < 0.9).astype(np.uint8) if masked else None
        if masked:
            keep[0] = 1
        return of(c, f"rows-{n}{'-masked' if masked else ''}", 0, keep)

    for what in ("tile-1", "tile", "tile+1", "round+1"):
        for masked in (False, True):
            def build(what=what, masked=masked):
                tile, rnd = layout()
                return seam({"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "round+1": rnd + 1}[what], masked)
            add(f"rows-{what}{'-masked' if masked else ''}", build)

    # past one sweep of the row grid and of the tile grid
    for what in PAST_SWEEP:
        for masked in (False, True):
            add(f"rows-{what}{'-masked' if masked else ''}",
                functools.partial(lambda what, masked: seam(past_sweep_rows(what), masked), what, masked))

    def packed_past_tiles():
        """Root 0 and, by the mask, the rows from 300 below the end of tile SWEEP_TILES - 1 on: every
        tile of the first tile round but the last counts 1 or 0, tile SWEEP_TILES counts its one row."""
        n = past_sweep_rows("tiles+1")
        first = n - 1 - 300
        c = synthetic(n, seed=7, packed_from=first)
        p = c.parent.copy()
        p[first] = 0
        return of(ExtractCase(c.name, c.state, c.ctrl, p), "rows-tiles+1-packed-by-mask", 0,
                  _mask(n, lambda r: (r == 0) | (r >= first)))

    add("rows-tiles+1-packed-by-mask", packed_past_tiles)

    def root_past_sweep(masked):
        c = seam(past_sweep_rows("2sweep+1"), masked)
        keep = c.keep
        if masked:
            keep = keep.copy()
            keep[SWEEP + 5] = 1
        return of(c, f"root-past-sweep{'-masked' if masked else ''}", SWEEP + 5, keep)

    add("root-past-sweep", functools.partial(root_past_sweep, False))
    add("root-past-sweep-masked", functools.partial(root_past_sweep, True))

    # masks over the main tree, root 0
    def masked_main(i):
        name, keep = masks_for(main_tree(), tc.busiest_row(*tc.MAIN))[i]
        return of(main_tree(), f"mask-{name}", 0, keep)

    for i, name in enumerate(("null", "ones", "zero", "root-only", "alternating", "bytes-2-0x80", "no-busiest")):
        add(f"mask-{name}", functools.partial(masked_main, i))

    def chain_cut():
        keep = np.ones(257, np.uint8)
        keep[128] = 0
        return of(chain(257), "mask-chain-cut", 0, keep)

    add("mask-chain-cut", chain_cut)

    def packed(masked):
        tile, _ = layout()
        n = 3 * tile + 17                          # the last tile is a partial one
        first = 3 * tile
        c = synthetic(n, seed=5, packed_from=first)
        keep = None
        if masked:                                 # the mask alone packs them: root 0, the first three tiles masked
            keep = _mask(n, lambda r: (r == 0) | (r >= first))
            p = c.parent.copy()
            p[first] = 0
            c = ExtractCase(c.name, c.state, c.ctrl, p)
        return of(c, f"mask-packed-last-tile{'-by-mask' if masked else ''}", 0 if masked else first, keep)

    add("mask-packed-last-tile", functools.partial(packed, False))
    add("mask-packed-last-tile-by-mask", functools.partial(packed, True))

    def lanes(which):
        tile, _ = layout()
        n = 2 * tile + 5
        hub = 0 if which == "first" else 63
        keep = _mask(n, lambda r: r % 64 == hub)
        return of(synthetic(n, seed=6, hub=hub), f"mask-{which}-lanes", hub, keep)

    add("mask-first-lanes", functools.partial(lanes, "first"))
    add("mask-last-lanes", functools.partial(lanes, "last"))

    # roots
    add("root-leaf", lambda: of(main_tree(), "root-leaf", a_leaf()))
    add("root-last", lambda: of(main_tree(), "root-last", len(main_tree().parent) - 1))
    add("root-busiest", lambda: of(main_tree(), "root-busiest", tc.busiest_row(*tc.MAIN)))
    add("root-busiest-alternating", lambda: of(main_tree(), "root-busiest-alternating", tc.busiest_row(*tc.MAIN),
                                               _mask(len(main_tree().parent), lambda r: r % 2 == tc.busiest_row(*tc.MAIN) % 2)))
    for r in D6_ROWS:
        add(f"root-d6-{r}", functools.partial(lambda r: of(tc.d6_case(), f"root-d6-{r}", r), r))
    add("d6", lambda: of(tc.d6_case(), "d6"))

    def masked_root():
        t = main_tree()
        keep = np.ones(len(t.parent), np.uint8)
        b = tc.busiest_row(*tc.MAIN)
        keep[b] = 0
        return of(t, "root-masked", b, keep)

    add("root-masked", masked_root)

    # crafted parents: on ordinary rows (root 0), and on the root itself
    for kind in tc.PARENT_KINDS:
        add(f"parent-{kind}", functools.partial(lambda k: of(tc.parent_case(k), f"parent-{k}"), kind))
        add(f"parent-{kind}-root-busiest",
            functools.partial(lambda k: of(tc.parent_case(k), f"parent-{k}-root-busiest", tc.busiest_row(*tc.MAIN)), kind))
        add(f"parent-{kind}-root-1", functools.partial(lambda k: of(tc.parent_case(k), f"parent-{k}-root-1", 1), kind))
    return out


CASES = all_cases()
IDS = [i for i, _ in CASES]
assert len(set(IDS)) == len(IDS)


@functools.lru_cache(maxsize=None)
def case(i) -> ExtractCase:
    return dict(CASES)[i]()

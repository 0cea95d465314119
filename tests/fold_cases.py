"""Crafted cases for the R2 key-log fold (k_fold_r2 through sbmp_fold_r2_batch, its host twin,
and the model of tests/fold_model.py).

A case is a ring [window][logSlots] of 16-bit keys, one S and one executed flag per iteration
from tFirst on, nR2, the rank and the prior table contents.  Fill policy: every ring starts as
random in-grid keys of both kinds (fixed seeds), so the slots >= S, the rows of unexecuted
iterations and the rows outside the window all hold keys that would count: a missing mask
changes a table.  The rows a case is about are then written over that.

Every constant of the kernel (window, keys per workgroup, largest nR2, the split of a log row)
is read from sbmp_fold_r2_info, none is written here.
"""
import functools
import zlib
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

from cudasbmp_amd import fold_r2_batch, fold_r2_info
from fold_model import fold_model

BLOCK = 256
INFO = fold_r2_info(BLOCK)
WINDOW, KEYS, MAX_R2, MAX_RANKS = INFO["window"], INFO["keysPerGroup"], INFO["maxR2"], INFO["maxRanks"]
INT_MAX = 2**31 - 1


def split(logSlots):
    i = fold_r2_info(logSlots)
    return i["groups"], i["per"]


@dataclass
class Case:
    name: str
    logSlots: int
    nR2: int
    tFirst: int
    S: list
    executed: list
    make_ring: Callable = field(repr=False)   # () -> (WINDOW, logSlots) uint16
    rank: int = 0
    nranks: int = 1
    prior: tuple = (0, 0)                     # R2Valid, R2Invalid start as these constants ...
    prior_cells: dict = field(default_factory=dict)   # ... except {cell: (valid, invalid)}

    def ring(self):
        r = self.make_ring()
        assert r.shape == (WINDOW, self.logSlots) and r.dtype == np.uint16
        return r

    def tables(self):
        v = np.full(self.nR2, self.prior[0], dtype=np.int32)
        i = np.full(self.nR2, self.prior[1], dtype=np.int32)
        for c, (pv, pi) in self.prior_cells.items():
            v[c], i[c] = pv, pi
        return v, i

    def rows(self):
        """(t, ring row) of the window's iterations."""
        return [(self.tFirst + j, (self.tFirst + j) % WINDOW) for j in range(len(self.S))]


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def keys(rng, shape, nR2, nokey=0.0):
    """Random in-grid keys of both kinds; a fraction `nokey` of them 0xffff."""
    k = (rng.integers(0, nR2, size=shape) | (rng.integers(0, 2, size=shape) << 15)).astype(np.uint16)
    if nokey:
        k[rng.random(size=shape) < nokey] = 0xffff
    return k


def base_ring(name, logSlots, nR2):
    return keys(rng_of("base:" + name), (WINDOW, logSlots), nR2)


def fresh_rows(case_name, logSlots, nR2, tFirst, S, executed, nokey=0.05):
    """The fill, then for every executed iteration fresh keys (5 % 0xffff) below its S."""
    def make():
        ring = base_ring(case_name, logSlots, nR2)
        rng = rng_of("rows:" + case_name)
        for j, (s, ex) in enumerate(zip(S, executed)):
            if ex:
                n = max(0, min(s, logSlots))
                ring[(tFirst + j) % WINDOW, :n] = keys(rng, n, nR2, nokey)
        return ring
    return make


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)
    return c


# ---------------------------------------------------------------- counter maximum
# KEYS keys of one kind in one cell: a packed half-word of the workgroup's histogram at its
# largest value, with no carry into the other half.
def _counter_ring(name, nR2, cell, kind, rows=1):
    def make():
        ring = base_ring(name, KEYS, nR2)
        for r in range(rows):
            if kind == "valid":
                ring[r, :] = cell | 0x8000
            elif kind == "invalid":
                ring[r, :] = cell
            else:
                ring[r, : KEYS // 2] = cell | 0x8000
                ring[r, KEYS // 2:] = cell
        return ring
    return make


for _kind in ("valid", "invalid", "half"):
    for _cn, _cell in (("cell0", 0), ("cellmax", 1023)):
        for _pn, _p in (("", 0), ("-prior7", 7), ("-priorbig", INT_MAX - KEYS)):
            _n = f"counter-{_kind}-{_cn}{_pn}"
            add(_n, KEYS, 1024, 0, [KEYS], [1], _counter_ring(_n, 1024, _cell, _kind),
                prior=(3, 5) if _p else (0, 0), prior_cells={_cell: (_p, _p)} if _p else {})
# two iterations of it in one call: the cell takes 2 KEYS > 2^16 through two workgroups
add("counter-two-iterations", KEYS, 1024, 0, [KEYS, KEYS], [1, 1],
    _counter_ring("counter-two-iterations", 1024, 1023, "valid", rows=2))

# ---------------------------------------------------------------- S around a piece, a block, a group border
BIG = 131072   # three ragged groups
BIG_GROUPS, BIG_PER = split(BIG)


def _shared_ring(name, logSlots, nR2):
    cache = {}

    def make():
        if "r" not in cache:   # one ring for the whole family: only S varies
            ring = base_ring(name, logSlots, nR2)
            ring[0] = keys(rng_of("rows:" + name), logSlots, nR2, 0.05)
            ring.flags.writeable = False
            cache["r"] = ring
        return cache["r"]
    return make


def _s_values(logSlots):
    return [("0", 0), ("1", 1), ("7", 7), ("8", 8), ("9", 9), ("255", 255), ("256", 256), ("257", 257),
            ("logSlots-1", logSlots - 1), ("logSlots", logSlots), ("logSlots+5", logSlots + 5)]


_small = _shared_ring("S-1024", 1024, 2304)
for _n, _s in _s_values(1024):
    add(f"S-1024-at-{_n}", 1024, 2304, 0, [_s], [1], _small)
_big = _shared_ring("S-big", BIG, 2304)
for _n, _s in _s_values(BIG) + [("per-1", BIG_PER - 1), ("per", BIG_PER), ("per+1", BIG_PER + 1),
                                ("per+8", BIG_PER + 8), ("2per-1", 2 * BIG_PER - 1), ("2per", 2 * BIG_PER),
                                ("2per+1", 2 * BIG_PER + 1), ("2per+8", 2 * BIG_PER + 8)]:
    add(f"S-big-at-{_n}", BIG, 2304, 0, [_s], [1], _big)

# ---------------------------------------------------------------- group shapes
GROUP_SHAPES = [BLOCK, KEYS, 65536, 2 * KEYS, 2 * KEYS + BLOCK, BIG]
for _ls in GROUP_SHAPES:
    _n = f"groups-{_ls}"
    add(_n, _ls, 2304, 0, [_ls], [1], fresh_rows(_n, _ls, 2304, 0, [_ls], [1]))

# ---------------------------------------------------------------- histogram sizes
OPT_IN_R2 = 65536 // 4 - 64   # nR2 + 64 sink words = 64 KB of dynamic LDS: the largest size without the opt-in
HIST_SIZES = [256, 1024, 8191, 8192, 8193, OPT_IN_R2, OPT_IN_R2 + 1, 30976, MAX_R2]


def _hist_ring(name, nR2):
    def make():
        ring = fresh_rows(name, 16384, nR2, 0, [16384, 16000], [1, 1])()
        for r in (0, 1):   # the last cell and the first, in both kinds
            ring[r, 5], ring[r, 6], ring[r, 7] = (nR2 - 1) | 0x8000, nR2 - 1, (nR2 - 1) | 0x8000
            ring[r, 8], ring[r, 9] = 0x8000, 0
        return ring
    return make


for _r2 in HIST_SIZES:
    _n = f"hist-{_r2}"
    add(_n, 16384, _r2, 0, [16384, 16000], [1, 1], _hist_ring(_n, _r2), prior=(1, 2))

# ---------------------------------------------------------------- dropped keys
DROPPED_CELLS = [0x7fff, 1024, 1025, 1024 + 63, 1024 + 64, 0x7ffe]   # at nR2 = 1024; 0x7fff | 0x8000 is 0xffff


def _dropped_ring():
    ring = base_ring("dropped-keys", 1024, 1024)
    rng = rng_of("rows:dropped-keys")
    row = keys(rng, 1024, 1024)
    drop = np.array([c | k for c in DROPPED_CELLS for k in (0, 0x8000)], dtype=np.uint16)
    where = rng.random(1024) < 0.4
    row[where] = rng.choice(drop, size=int(where.sum()))
    row[:len(drop)] = drop   # every one of them at least once
    ring[0] = row
    return ring


add("dropped-keys", 1024, 1024, 0, [1024], [1], _dropped_ring, prior=(1, 1))

# ---------------------------------------------------------------- windows
def _window_S(name, T):
    """One S per iteration in [0, 1024]: every residue mod 8, and most of them far below the
    1,024 in-grid keys the row holds from before."""
    rng = rng_of("S:" + name)
    S = [int(8 * rng.integers(0, 120) + (j % 8)) for j in range(T)]
    if T >= 8:
        S[3], S[5] = 1024, 0
    return S


def _window(name, tFirst, T, unexecuted=()):
    S = _window_S(name, T)
    ex = [0 if (tFirst + j) in unexecuted else 1 for j in range(T)]
    return add(name, 1024, 2304, tFirst, S, ex, fresh_rows(name, 1024, 2304, tFirst, S, ex), prior=(2, 1))


_window("window-0-1", 0, 1)
_window("window-0-64", 0, WINDOW)
_window("window-40-64", 40, WINDOW)                       # rows 40 .. 63, then 0 .. 39
_window("window-127-1", 2 * WINDOW - 1, 1)
_window("window-31-64-holes", 31, WINDOW, unexecuted=set(range(50, 58)) | {31 + WINDOW - 1})
_window("window-none-executed", 5, WINDOW, unexecuted=set(range(5, 5 + WINDOW)))

# ---------------------------------------------------------------- ranks
RANK_BLOCKS = 24
RANK_OFFSETS = [0, 1, 7, 8, 9, 255]
RANK_GROUPS = {}   # P -> (the global single-rank case, the P rank cases)


def _rank_family(P):
    per_rank = RANK_BLOCKS // P
    # S on a block of each rank at each offset: rank r's local block b is global block r + P b
    S = [(r + P * ((o + r) % per_rank)) * BLOCK + off for r in range(P) for o, off in enumerate(RANK_OFFSETS)]
    T = len(S)
    assert T <= WINDOW
    gname = f"ranks-P{P}-global"
    gmake = fresh_rows(gname, RANK_BLOCKS * BLOCK, 2304, 0, S, [1] * T)
    g = add(gname, RANK_BLOCKS * BLOCK, 2304, 0, S, [1] * T, gmake, prior=(4, 9))

    def local(r):
        def make():   # the global blocks r, r + P, r + 2 P, ... in that order
            ring = gmake().reshape(WINDOW, RANK_BLOCKS, BLOCK)
            return np.ascontiguousarray(ring[:, r::P, :]).reshape(WINDOW, per_rank * BLOCK)
        return make
    ranks = [add(f"ranks-P{P}-r{r}", per_rank * BLOCK, 2304, 0, S, [1] * T, local(r), rank=r, nranks=P, prior=(4, 9))
             for r in range(P)]
    RANK_GROUPS[P] = (g, ranks)


for _P in (2, 3, MAX_RANKS):
    _rank_family(_P)

BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- the references, computed once
@functools.lru_cache(maxsize=None)
def model(name):
    """The model's tables for a case, computed once and shared (read-only)."""
    c = BY_NAME[name]
    v, i = c.tables()
    out = fold_model(c.ring(), c.S, c.executed, c.tFirst, c.nR2, rank=c.rank, nranks=c.nranks, R2Valid=v, R2Invalid=i)
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def twin(name, repeat=1):
    c = BY_NAME[name]
    v, i = c.tables()
    return fold_r2_batch(c.ring(), c.S, c.executed, c.tFirst, c.nR2, rank=c.rank, nranks=c.nranks, R2Valid=v,
                         R2Invalid=i, device=False, repeat=repeat)


def same(got, want):
    return all(np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64)) for g, w in zip(got, want))

"""The goal-query cases of tests/tree_query_cases.py, proven on the CPU alone: a correct query
passes every one of them, and each of a list of wrong queries, written here in numpy, is caught.

query() states the goal query a second time (include/sbmp/tree_query.h), with switches that each
break it the way a kernel could be broken:

  mask-ignored-nearest    nearestRow taken over every row, dead ones included
  mask-ignored-inside     count, firstRow and bestRow taken over every row
  mask-equals-1           a row alive iff its byte == 1 (the rule is != 0)
  highest-on-equal-d2     the highest row kept among rows of equal d2
  highest-on-equal-cost   the highest row kept among inside rows of equal cost
  strict-threshold        d2 < t(r) in place of d2 <= t(r)
  past-sweep-dropped      the rows at or past 524,288 never read (no second sweep)
  partial-block-dropped   the rows of the last, partial block of 256 never read
  tile-at-goal-0          every tile of the ladder writes its answers at goal 0 upward, not
                          at its own first goal upward; the goals nothing wrote stay empty
  dead-cost-admitted      a dead inside row's cost admitted to bestRow / bestCost
  empty-set-row-0         with no alive row, nearestRow 0 and row 0's distance
  nan-lowest              a NaN d2 taken as the lowest (np.argmin's order)

A wrong query is caught by a case when its answers differ from the model's in any field of any
goal.  CAUGHT_BY names, for every wrong query, cases built to catch it, and each must; beyond
that every wrong query must be caught at least once and every masked case must catch at least
one of them, which is asserted over the whole table: 12 of 12 wrong queries caught, no idle case.
The unmasked single-4194381 is left out of the table for its size (it has its own test in
tests/test_tree_query.py); the table takes every other case.
"""
import numpy as np
import pytest

import tree_query_cases as tc
from tree_query_model import FIELDS, assert_same_answers, d2_of, empty_answers, inside_of

WRONG = ("mask-ignored-nearest", "mask-ignored-inside", "mask-equals-1", "highest-on-equal-d2", "highest-on-equal-cost",
         "strict-threshold", "past-sweep-dropped", "partial-block-dropped", "tile-at-goal-0", "dead-cost-admitted",
         "empty-set-row-0", "nan-lowest")

CAUGHT_BY = {
    "mask-ignored-nearest": ("masked-ties", "masked-zero-distance", "masked-rows-257", "masked-rows-1048577"),
    "mask-ignored-inside": ("masked-ties", "masked-radius-edges", "masked-zero-distance", "masked-one-256",
                            "masked-rows-524365"),
    "mask-equals-1": ("masked-bytes",),
    "highest-on-equal-d2": ("masked-ties", "ties"),
    "highest-on-equal-cost": ("masked-ties", "ties"),
    "strict-threshold": ("masked-radius-edges", "radius-edges", "masked-zero-distance", "zero-distance"),
    "past-sweep-dropped": ("masked-rows-524365", "masked-rows-1048577"),
    "partial-block-dropped": ("masked-rows-257", "masked-rows-524365", "masked-rows-1048577", "masked-one-699"),
    "tile-at-goal-0": ("masked-goals-9", "masked-goals-12", "masked-goals-13", "masked-goals-16", "masked-goals-17",
                       "masked-goals-65", "masked-goals-5", "masked-goals-7", "tiles-17", "tiles-18"),
    "dead-cost-admitted": ("masked-ties", "masked-nonfinite"),
    "empty-set-row-0": ("masked-none",),
    "nan-lowest": ("masked-nonfinite", "nonfinite"),
}


def _ladder(Q: int, masked: bool):
    """(first, n) of every launch: tiles of 8, 4, 1 for the masked query; whole tiles of 16, then
    the smallest of 8, 4, 2, 1 that holds the rest, for the unmasked one."""
    out, first = [], 0
    while first < Q:
        left = Q - first
        n = (8 if left >= 8 else 4 if left >= 4 else 1) if masked else min(left, 16)
        out.append((first, n))
        first += n
    return out


def _lowest(bits, rows, highest_row: bool) -> int:
    """The row of the lowest bits; among equals the lowest row, or the highest."""
    lowest = rows[bits == bits.min()]
    return int(lowest.max() if highest_row else lowest.min())


def query(state, ctrl, goals, alive=None, wrong=()) -> dict:
    x, y, cost = state[:, 0], state[:, 1], ctrl[:, 3]
    R, Q = len(x), len(goals)
    every = np.ones(R, bool)
    live = every.copy() if alive is None else (alive == 1 if "mask-equals-1" in wrong else alive != 0)
    if "past-sweep-dropped" in wrong:
        live[tc.SWEEP:] = False
    if "partial-block-dropped" in wrong and R % 256:
        live[R - R % 256:] = False
    near_live = every if "mask-ignored-nearest" in wrong else live
    in_live = every if "mask-ignored-inside" in wrong else live
    best_live = every if "dead-cost-admitted" in wrong else in_live
    out = empty_answers(Q)
    for q, (gx, gy, r) in enumerate(goals):
        d2 = d2_of(x, y, gx, gy)
        ins = inside_of(d2, r)
        if "strict-threshold" in wrong:   # d2 < t(r): the next float above d2 is inside too
            ins &= inside_of(np.nextafter(d2, np.float32(np.inf)), r)
        rows = np.flatnonzero(ins & in_live)
        out["count"][q] = len(rows)
        if len(rows):
            out["firstRow"][q] = rows[0]
            rows = np.flatnonzero(ins & best_live)
            b = _lowest(cost[rows].view(np.uint32), rows, "highest-on-equal-cost" in wrong)
            out["bestRow"][q], out["bestCost"][q] = b, cost[b]
        rows = np.flatnonzero(near_live)
        k = -1
        if len(rows):
            if "nan-lowest" in wrong:
                with np.errstate(all="ignore"):
                    k = int(rows[np.argmin(d2[rows])])
            else:
                k = _lowest(d2[rows].view(np.uint32), rows, "highest-on-equal-d2" in wrong)
        elif "empty-set-row-0" in wrong:
            k = 0
        if k >= 0:
            out["nearestRow"][q] = k
            with np.errstate(all="ignore"):
                out["nearestDistance"][q] = np.sqrt(d2[k], dtype=np.float32)
    if "tile-at-goal-0" in wrong:
        moved = empty_answers(Q)
        for first, n in _ladder(Q, alive is not None):
            for f in FIELDS:
                moved[f][:n] = out[f][first:first + n]
        out = moved
    return out


def _same(a: dict, b: dict) -> bool:
    return all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in FIELDS)


def _case(name):
    """(state, ctrl, goals, mask or None, expect, model)"""
    if name in tc.MASKED_BUILDERS:
        c = tc.masked_case(name)
        return c.state, c.ctrl, c.goals, c.mask, c.expect, c.model
    state, ctrl, goals, expect, model = tc.case(name)
    return state, ctrl, goals, None, expect, model


TABLE_CASES = tuple(n for n in tc.NAMES if n != f"single-{tc.BIG}") + tc.MASKED_NAMES


@pytest.mark.parametrize("name", TABLE_CASES)
def test_the_true_query_passes(name):
    state, ctrl, goals, mask, expect, model = _case(name)
    got = query(state, ctrl, goals, mask)
    assert_same_answers(got, model, label=name)
    tc.check_expect(got, expect, label=name)


def test_ladders():
    assert _ladder(13, True) == [(0, 8), (8, 4), (12, 1)] and _ladder(7, True) == [(0, 4), (4, 1), (5, 1), (6, 1)]
    assert _ladder(17, True) == [(0, 8), (8, 8), (16, 1)] and _ladder(18, False) == [(0, 16), (16, 2)]
    # every composition of the masked ladder: each tile alone, repeated, and behind each of the others
    shapes = {tuple(n for _, n in _ladder(Q, True)) for Q in tc.MASKED_GOAL_COUNTS}
    assert {(1,), (4,), (8,), (1, 1), (8, 8), (4, 1), (8, 1), (8, 4), (8, 4, 1), (8, 8, 1)} <= shapes
    assert (4, 1, 1, 1) in shapes and tuple([8] * 8 + [1]) in shapes


@pytest.fixture(scope="module")
def table():
    """{(wrong, case): caught}"""
    t = {}
    for name in TABLE_CASES:
        state, ctrl, goals, mask, _, model = _case(name)
        for w in WRONG:
            t[w, name] = not _same(query(state, ctrl, goals, mask, wrong=(w,)), model)
    return t


@pytest.mark.parametrize("w", WRONG)
def test_wrong_query_is_caught(w, table):
    by = [n for n in TABLE_CASES if table[w, n]]
    print(w, "caught by", by)
    assert by, f"nothing catches {w}"
    missed = [n for n in CAUGHT_BY[w] if not table[w, n]]
    assert not missed, f"{w} passes {missed}, which were built to catch it"


def test_every_wrong_query_is_caught_and_every_masked_case_is_useful(table):
    caught = [w for w in WRONG if any(table[w, n] for n in TABLE_CASES)]
    idle = [n for n in tc.MASKED_NAMES if not any(table[w, n] for w in WRONG)]
    print(f"{len(caught)} of {len(WRONG)} wrong queries caught; idle masked cases: {idle}")
    assert set(CAUGHT_BY) == set(WRONG) and len(WRONG) == 12
    assert len(caught) == len(WRONG)
    assert not idle, f"masked cases that catch no wrong query: {idle}"
    for name in ("nonfinite",) + tuple(f"tiles-{Q}" for Q in tc.TILE_COUNTS if Q > 16):
        assert any(table[w, name] for w in WRONG), name

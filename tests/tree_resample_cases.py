"""The crafted trees of the resample tests (tests/test_tree_resample.py on the host twin,
tests/test_gpu_tree_resample.py on the kernels); the grown trees, the chains and the star are
tests/tree_recheck_cases.py's.  A case is that module's Case (state, ctrl, parent, params); the
boxes play no part here.

  chain(L)        a single chain of L rows (L = 1: the root alone), every edge 0.07 s
  pow2(rows)      a chain whose edges all last 1.0 s with numDisc = 8: dt = 0.125 exactly, so with
                  period 0.125 every grid time is a step boundary, with period 1.0 an edge boundary
  bad_durations   a chain whose edges last (the smallest denormal), 0.3, 0, 0.2, -1, NaN, 0.25,
                  +inf, 0.4 seconds
  rounding        one edge and a period whose last grid time rounds to more than the path's time
  many_requests   about 700 requests whose samples together pass one sweep of k_path_resample's grid
"""
from __future__ import annotations

import functools

import numpy as np

import tree_recheck_cases as tc
from tree_paths_model import euler_steps
from tree_query_cases import SWEEP

PERIODS = (0.05, 0.013, float(np.float32(1.05) / np.float32(10)))
PERIOD_IDS = ("p0.05", "p0.013", "p0.105f")
CHAIN_LENGTHS = (1, 2, 3, 64, 65, 257)
COUNTS = (1, 63, 64, 65, 255, 256, 257)
KEYS = ("numDisc", "agentLength", "agent")

# found by a search over 4,000 float32 durations d of [0.06, 1.05) with period = d / 11 in
# double: floor(d / period) = 11 and fl(11 * period) = d + one double ulp > d
ROUNDING_DURATION = np.array([0x3F724D6A], np.uint32).view(np.float32)[0]
ROUNDING_PERIOD = float.fromhex("0x1.60709a2e8ba2fp-4")
ROUNDING_GRID = 11


def params_of(case) -> dict:
    return {k: case.params[k] for k in KEYS}


def nodes_of(case) -> np.ndarray:
    """Every 97th row plus the last."""
    R = len(case.parent)
    return np.append(np.arange(0, R, 97), R - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def chain(L) -> tc.Case:
    return tc.chain_case(max(L - 1, 1), "last").prefix(L, f"resample-chain-{L}")


def _chain_from(name, root, controls, params, hold=()) -> tc.Case:
    """Row r the child of row r - 1 under controls[r - 1], each stored state the model's own trace
    of its edge; a row of `hold` (a duration that is no time) keeps its parent's state."""
    n = len(controls) + 1
    state = np.zeros((n, 4), np.float32)
    ctrl = np.zeros((n, 4), np.float32)
    state[0] = root
    ctrl[1:, :3] = controls
    for r in range(1, n):
        if r in hold:
            state[r] = state[r - 1]
        else:
            state[r] = euler_steps(state[r - 1][None], ctrl[r, :3][None], params["numDisc"], params["agentLength"],
                                   params["agent"])[0, -1]
    return tc.Case(name, state, ctrl, np.arange(-1, n - 1, dtype=np.int32), np.zeros((0, 4), np.float32),
                   dict(tc.CHAIN_PARAMS, **params))


@functools.lru_cache(maxsize=None)
def pow2(rows=7, agent="car") -> tc.Case:
    c = [((1.0 if r % 2 else -1.0), 0.05 * r, 1.0) for r in range(1, rows)]
    if agent == "point":
        c = [(0.25 * (1 + r % 3), -0.125 * (r % 2) + 0.0625, 1.0) for r in range(1, rows)]
    return _chain_from(f"pow2-{agent}-{rows}", (1.0, 5.0, 0.0, 1.0), c, dict(numDisc=8, agentLength=1.0, agent=agent))


BAD_DURATIONS = (np.float32(1e-45), 0.3, 0.0, 0.2, -1.0, np.nan, 0.25, np.inf, 0.4)
BAD_ROWS = (3, 5, 6, 8)          # the rows whose durations are 0, -1, NaN and +inf
DENORMAL_ROW = 1


@functools.lru_cache(maxsize=None)
def bad_durations() -> tc.Case:
    c = [((1.0 if r % 2 else -1.0), 0.1, d) for r, d in enumerate(BAD_DURATIONS, start=1)]
    return _chain_from("bad-durations", (1.0, 5.0, 0.3, 1.0), c, dict(numDisc=10, agentLength=1.0, agent="car"),
                       hold=BAD_ROWS)


@functools.lru_cache(maxsize=None)
def rounding() -> tc.Case:
    return _chain_from("rounding", (1.0, 5.0, 0.3, 1.0), [(1.0, 0.1, ROUNDING_DURATION)],
                       dict(numDisc=10, agentLength=1.0, agent="car"))


def period_for_total(T, total) -> float:
    """A period that gives a path of time T exactly `total` >= 2 samples: floor(T / period) =
    total - 2, aimed at the middle of that interval."""
    return float(T) / (total - 2 + 0.5)


MANY_REQUESTS = 700


@functools.lru_cache(maxsize=None)
def many_requests():
    """(case, nodes, period): about 700 distinct rows of the main grown tree with crafted -1 parents
    (tests/tree_recheck_cases.py: the busiest row's descendants have broken paths), every 50th
    request -1, and a period that puts the sample total between SWEEP + 1,000 and 1.2 SWEEP, so
    the samples of k_path_resample's later sweeps belong to the last requests."""
    from tree_paths_model import OK, path_of
    from tree_resample_model import clock_of
    case = tc.parent_case("minus1")
    R = len(case.parent)
    busiest = tc.busiest_row(*tc.MAIN)
    below = np.flatnonzero(tc.grown(*tc.MAIN).parent == busiest)[:3]
    nodes = np.unique(np.concatenate([np.arange(1, R, R // MANY_REQUESTS), [busiest, R - 1], below])).astype(np.int32)
    nodes[::50] = -1
    par = case.parent.tolist()
    times = [clock_of(case.ctrl, chain)[-1] for st, chain in (path_of(par, int(n), R) for n in nodes) if st == OK]
    # sum of floor(T_i / period) + 2 over the ok requests, aimed at 1.1 SWEEP: floor loses half a sample a path
    period = period_for_total(sum(times), int(1.1 * SWEEP - 1.5 * len(times)))
    return case, nodes, period

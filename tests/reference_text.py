"""The reference's own per-child functions, host-compiled (oracle/_ref/libkgmt_ref.so, built by
`make -C oracle ref` from the reference tree; oracle/ref_shim holds the recipe's own text), and
what the tests of tests/test_reference_text.py and tests/test_gpu_reference_text.py share:

  lib()            the loader.  With the reference tree present the library is (re)built; without
                   it an already built one is used; a missing one is an error, never a skip.
  before,          one iteration of a stepped planner (the CPU oracle or the HIP planner alike)
  check_step       fed slot by slot to the reference's propagateAndCheck, getR1 and getR2: the
                   state read before the step, and the check after it.
  replay_step      both round one step of the planner itself (a batch steps its members together).
  replay           replay_step over a whole run, with the slot count and the valid share.
  goal_band        which points lie so near the goal circle that the float rule (D18) and the
                   reference's text under g++ (a double distance) may differ.

The oracle, the float64 model and the kernels are this project's reading of the reference; the
functions called here are the reference's text.  What stays outside: cuRAND's seeding constants,
libdevice's sin / cos / tan bits (D9's functions stand in), nvcc's contraction choices (g++'s
-ffp-contract=fast stands in) and the __global__ kernels.

A plain module: no fixtures, no GPU, nothing at import but numpy.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from region_scenarios import R1_KEYS, R2_KEYS, counters, xorwow_step

U32 = np.uint32
F32 = np.float32
F64 = np.float64


def lib():
    from oracle import pyoracle
    pyoracle.ref_lib()
    return pyoracle


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


# ---------------------------------------------------------------- the replay
def planner_args(sc) -> dict:
    """propagateAndCheck's scalar arguments for a Scenario."""
    cfg, _ = sc.config()
    return dict(numDisc=cfg["numDisc"], agentLength=cfg["agentLength"], width=cfg["width"], height=cfg["height"])


def is_car(sc) -> bool:
    return sc.config()[1].get("agent", "car") == "car"


def _logs(p):
    return p.iter_logs() if hasattr(p, "iter_logs") else p.iter_log()


def _step(p) -> bool:
    return bool(p.step() if hasattr(p, "iter_logs") else p.step(1))


@dataclass(frozen=True, eq=False)
class Step:
    """One replayed iteration: the slots, the reference's children and verdicts."""
    S: int
    children: np.ndarray
    valid: np.ndarray
    more: bool


@dataclass(frozen=True, eq=False)
class Before:
    """What a check of one iteration needs from before it."""
    rng: np.ndarray
    done: int
    regions: dict


def before(p) -> Before:
    return Before(p.rng().copy(), len(_logs(p)), p.regions())


def cell_sizes(sc):
    """(R1Size, N, R2Size, n) as KGMT's constructor computes them (KGMT.cu:13-14)."""
    cfg, _ = sc.config()
    W, N, n = F32(cfg["width"]), int(cfg["N"]), int(cfg["n"])
    return F32(W / F32(N)), N, F32(W / F32(n * N)), n


def check_step(p, sc, b: Before, more: bool, obstacles=None, label="") -> Step | None:
    """Hold the iteration `p` ran since `b` to the reference's text.  Slot s is (tree[uParent[s]], the
    RNG state read before the step), fed to propagateAndCheck.
      - The stored child must be the reference's, bit for bit.
      - The stored RNG state must be the reference's three draws on, and a fourth (the accept draw,
        KGMT.cu:395) exactly where the reference's verdict is true: that is how a stepped planner shows
        its own verdict per slot, so a slot the planner treats as unusable is one the reference's text
        calls invalid (it left the workspace or met a box), and the other way round.
      - The region counters must have moved by the reference's getR1 / getR2 of those children under the
        reference's verdicts (KGMT.cu:392-411 with D3: a cell of -1 is not counted).
    None when no iteration ran."""
    po = lib()
    obs = sc.obstacles() if obstacles is None else obstacles
    logs = _logs(p)
    if len(logs) == b.done:
        return None
    assert len(logs) == b.done + 1, label
    S = int(logs[-1][5])
    u, uParent = p.unexplored()
    tree = p.tree()[0]
    assert S <= len(b.rng) and (uParent[:S] >= 0).all() and (uParent[:S] < int(logs[-1][1])).all(), label
    r = po.ref_expand(tree[uParent[:S]], b.rng[:S], obs, **planner_args(sc))
    diff = np.nonzero((bits(u[:S]) != bits(r["children"])).any(axis=1))[0]
    assert len(diff) == 0, f"{label}: {len(diff)} of {S} children differ from the reference's text, first slots {diff[:8]}"
    drawn4 = xorwow_step(r["rng"])[1]
    want = np.where(r["valid"][:, None], drawn4, r["rng"])
    rng_after = p.rng()
    bad = np.nonzero((rng_after[:S] != want).any(axis=1))[0]
    assert len(bad) == 0, (f"{label}: {len(bad)} of {S} slots hold another verdict than the reference's text "
                           f"(or other draws), first slots {bad[:8]}")
    assert np.array_equal(rng_after[S:], b.rng[S:]), f"{label}: RNG states past S moved"
    # the cells: the children are finite and x / R1Size is far inside int range, where the conversion is defined
    R1Size, N, R2Size, n = cell_sizes(sc)
    xy = np.ascontiguousarray(r["children"][:, :2])
    assert np.isfinite(xy).all() and (np.abs(xy / R1Size) < 2.0 ** 31).all(), label
    r1, r2 = po.ref_cells(xy, R1Size, N, R2Size, n)
    after = p.regions()
    count = counters(b.regions, r1.astype(np.int64), r2.astype(np.int64), r["valid"], n)
    for k in R1_KEYS + R2_KEYS:
        assert np.array_equal(after[k], count[k]), f"{label}: {k} differs at cells {np.nonzero(after[k] != count[k])[0][:8]}"
    return Step(S, r["children"], r["valid"], more)


def replay_step(p, sc, obstacles=None, label="") -> Step | None:
    """Step `p` (the CPU oracle or the HIP planner) once and check_step the iteration."""
    b = before(p)
    return check_step(p, sc, b, _step(p), obstacles, label)


def left_workspace(sc, children):
    """statePropagator.cu:42 on the stored end point: a child that leaves keeps the (x, y) it left with."""
    a = planner_args(sc)
    x, y = children[:, 0], children[:, 1]
    with np.errstate(invalid="ignore"):
        return (x <= 0) | (x >= F32(a["width"])) | (y <= 0) | (y >= F32(a["height"]))


@dataclass(frozen=True, eq=False)
class Replay:
    iterations: int
    slots: int
    valid: int
    first: Step | None      # iteration 1 (the root's children)

    @property
    def share(self) -> float:
        return self.valid / max(1, self.slots)


def replay(p, sc, obstacles=None, iterations=None, label="") -> Replay:
    """replay_step until the planner stops (or `iterations` ran).  replay_step has shown that the
    planner calls a child unusable exactly where the reference's text does; here, besides, no child the
    reference calls valid has left the workspace."""
    n = slots = valid = 0
    first = None
    while iterations is None or n < iterations:
        st = replay_step(p, sc, obstacles, f"{label or sc.name} iteration {n + 1}")
        if st is None:
            break
        n += 1
        first = first or st
        slots += st.S
        valid += int(st.valid.sum())
        assert not (st.valid & left_workspace(sc, st.children)).any(), f"{label}: a valid child outside the workspace"
        if not st.more:
            break
    return Replay(n, slots, valid, first)


# ---------------------------------------------------------------- the goal band
GOAL_BAND_ULPS = 3


def goal_distance64(xy, goal):
    """The distance in float64 from the float32 coordinates (the differences are exact in float64)."""
    xy = np.asarray(xy, dtype=F32).astype(F64)
    return np.hypot(xy[:, 0] - F64(F32(goal[0])), xy[:, 1] - F64(F32(goal[1])))


def goal_band(xy, goal, r, ulps=GOAL_BAND_ULPS):
    """True where the float64 distance lies within `ulps` float32 ulps of r from r.  Outside this band
    the float rule sqrtf(dx dx + dy dy) < r (D18) and a double evaluation must agree: the float route's
    roundings (the two differences are shared; the squares, the sum and the root) stay under 2 ulp of
    the distance, the third ulp covers the double route's own final rounding and this yardstick."""
    r = F32(r)
    ulp = F64(np.spacing(r))
    return np.abs(goal_distance64(xy, goal) - F64(r)) <= ulps * ulp

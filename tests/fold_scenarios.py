"""Scenario table for the fold inside long runs (family K): plans that pass the
64-iteration window of the R2 key log with a slot count S that varies, so that ring row t % 64
still holds, at and past S(t), the keys iteration t - 64 logged there.

Base: the demo scene and car, goalThreshold = 0 (the loop never ends at the goal), the
reference batch rule, 140 iterations, samplesPerIteration = 1000, maxTreeSize = 150000: S lies
between 0 and 1000 and changes from iteration to iteration.  tests/test_fold_scenarios_oracle.py
asserts on the CPU oracle alone what each scenario reaches (coverage()); the GPU forms are in
tests/test_gpu_fold_scenarios.py.

Plain numpy: no GPU and no oracle at import.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, OBSTACLES_CSV

WINDOW = 64   # the fold's window as the scenarios were chosen for; the tests compare it with sbmp_fold_r2_info
ITERATIONS = 140
LOG = {n: i for i, n in enumerate(("itr", "treeSizeBefore", "nG", "k", "nExp", "S", "A", "treeSizeAfter", "goalIdx"))}


@dataclass(frozen=True)
class Scenario:
    name: str
    seed: int
    n: int = 8
    samplesPerIteration: int = 1000
    maxTreeSize: int = 150000
    min_stale: int = 2          # the floor of condition (a) for this scenario
    min_residues: int = 1

    def config(self):
        """(cfg, extra): the KGMT positional configuration and its keyword extras."""
        cfg = dict(DEMO)
        cfg.update(n=self.n, numIterations=ITERATIONS, maxTreeSize=self.maxTreeSize, goalThreshold=0.0)
        return cfg, dict(samplesPerIteration=self.samplesPerIteration, batchRule="reference")

    def with_seed(self, seed):
        return Scenario(f"{self.name}-seed{seed}", seed, self.n, self.samplesPerIteration, self.maxTreeSize, 0, 0)

    @property
    def nR2(self):
        return 256 * self.n * self.n


# the base (seed 11: 2 iterations meet condition (a)) and the best of a search over seeds 1 .. 39 and
# samplesPerIteration 1000 / 1500 / 3000 for at least 4 such iterations with at least 3 residues of S mod 8
BASE = Scenario("K-base", 11)
BEST = Scenario("K-best", 34, min_stale=4, min_residues=3)
# n = 3 keeps so few parents at samplesPerIteration = 1000 (S stays at 160 or 192 from iteration 27 on, all
# multiples of 32) that no seed of 1 .. 99 gave one such iteration; at 128 the cap cuts S, and seed 34 gives 4
SCENARIOS = [BASE, BEST, Scenario("K-best-n11", 34, n=11), Scenario("K-best-n3", 34, n=3, samplesPerIteration=128)]
BY_NAME = {s.name: s for s in SCENARIOS}
IDS = [s.name for s in SCENARIOS]


def obstacles() -> np.ndarray:
    return np.loadtxt(OBSTACLES_CSV, delimiter=",", dtype=np.float32).reshape(-1, 4)


def make_oracle(sc: Scenario, iterations=None, threads: int = 8):
    """The CPU oracle on a scenario, stepped `iterations` times (None: to the end of the plan)."""
    from oracle.pyoracle import Oracle, PlannerConfig
    cfg, extra = sc.config()
    o = Oracle(PlannerConfig(**cfg, samplesPerIteration=extra["samplesPerIteration"], batchRule=0), threads=threads)
    o.begin(DEMO_INITIAL, DEMO_GOAL, obstacles(), sc.seed)
    done = 0
    while (iterations is None or done < iterations) and o.step():
        done += 1
    return o


@functools.lru_cache(maxsize=None)
def oracle_at(name: str, iterations=None, seed=None):
    """Shared, read-only: the oracle of scenario `name` (under another seed, if given) after
    `iterations` steps."""
    sc = BY_NAME[name]
    return make_oracle(sc if seed is None else sc.with_seed(seed), iterations)


def coverage(sc: Scenario) -> dict:
    """What the oracle says the scenario reaches.  Iteration t logs into ring row t % WINDOW.
    stale: the iterations t > WINDOW with S(t) < S(t - WINDOW) and S(t) % 8 != 0 (the row holds keys
    of t - WINDOW at and past S(t), and the 8-key piece at S(t) straddles it); counting: those
    among them where a slot of [S(t), S(t - WINDOW)) holds, from iteration t - WINDOW, a child
    inside the workspace, whose key a fold without the S mask would count."""
    from oracle.pyoracle import Oracle, PlannerConfig
    cfg, extra = sc.config()
    o = Oracle(PlannerConfig(**cfg, samplesPerIteration=extra["samplesPerIteration"], batchRule=0), threads=8)
    o.begin(DEMO_INITIAL, DEMO_GOAL, obstacles(), sc.seed)
    S, inside = {}, {}
    while o.step():
        row = o.iter_logs()[-1]
        t, s = int(row[LOG["itr"]]), int(row[LOG["S"]])
        u, _ = o.unexplored()
        S[t] = s
        x, y = u[:s, 0], u[:s, 1]
        inside[t] = (x >= 0.0) & (x < cfg["width"]) & (y >= 0.0) & (y < cfg["height"])
    stale = [t for t in sorted(S) if t - WINDOW in S and S[t] < S[t - WINDOW] and S[t] % 8 != 0]
    counting = [t for t in stale if np.any(inside[t - WINDOW][S[t]:])]
    r = o.regions()
    return {"executed": len(S), "stale": stale, "residues": sorted({S[t] % 8 for t in stale}), "counting": counting,
            "nonzero_cells": int(np.count_nonzero(r["R2Valid"].astype(np.int64) + r["R2Invalid"])),
            "S_min": min(S.values()), "S_max": max(S.values()), "nR2": len(r["R2Valid"])}

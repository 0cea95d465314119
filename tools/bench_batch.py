"""Queries per second of KGMTBatch against consecutive KGMT.plan calls on one handle.

    python tools/bench_batch.py [--pairs 7] [--warmup 2] [--sizes 1,4,8] [--out profiles/batch/bench_batch.json]

Workload: the reference demo (demos/main.cu:19-46) for seeds 1..B.  Batched run:
KGMTBatch.plan of the B queries.  Baseline: the same B queries as consecutive KGMT.plan
calls on one handle (the single-planner path).  Both are host wall time around the calls,
begin() included.  A/B practice (profiles/r06/*/ab.txt): warm-up runs first, then
interleaved pairs (baseline, batch, baseline, batch, ...), medians with the spread
(min .. max) reported.  B values: --sizes plus the largest B that still gives one launch
per iteration (read from info() of a batch of one).  Both sides' results are compared
(iterations, tree size, goal row per seed), so a faster wrong answer cannot pass.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEMO = dict(width=20.0, height=20.0, N=16, n=8, numIterations=100, maxTreeSize=30000, numDisc=10,
            agentLength=1.0, goalThreshold=0.5)
INITIAL = (5.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0)
GOAL = (2.0, 18.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_batch.json"))
    a = ap.parse_args()
    if a.pairs < 5:
        ap.error("at least five interleaved pairs")

    from cudasbmp_amd import KGMT, KGMTBatch, DeviceBuffer, read_obstacles_csv
    obs = read_obstacles_csv(os.path.join(ROOT, "configurations", "obstacles", "obstacles.csv"))
    d_obs = DeviceBuffer(obs)

    one = KGMTBatch(1, **DEMO)
    one.plan([INITIAL], [GOAL], d_obs, len(obs), [1])
    i1 = one.info()
    largest = i1["residentGroups"] // i1["groupsPerMember"]
    sizes = sorted(set([int(x) for x in a.sizes.split(",") if x] + [largest]))
    single = KGMT(**DEMO)
    rows = []
    for B in sizes:
        seeds = list(range(1, B + 1))
        batch = KGMTBatch(B, **DEMO)

        def run_single():
            t0 = time.perf_counter()
            res = [single.plan(INITIAL, GOAL, d_obs, len(obs), seed=s) for s in seeds]
            return time.perf_counter() - t0, [(r.iterations, r.treeSize, r.goalIndex) for r in res]

        def run_batch():
            t0 = time.perf_counter()
            res = batch.plan([INITIAL] * B, [GOAL] * B, d_obs, len(obs), seeds)
            return time.perf_counter() - t0, [(r.iterations, r.treeSize, r.goalIndex) for r in res]

        for _ in range(a.warmup):
            _, want = run_single()
            _, got = run_batch()
            assert got == want, f"B={B}: the batch's results differ from the single plans'"
        ts, tb = [], []
        for _ in range(a.pairs):
            t, want = run_single()
            ts.append(t)
            t, got = run_batch()
            tb.append(t)
            assert got == want, f"B={B}: the batch's results differ from the single plans'"
        info = batch.info()
        iters = [w[0] for w in want]
        ms, mb = statistics.median(ts), statistics.median(tb)
        row = {
            "B": B, "pairs": a.pairs, "launchesPerIteration": info["launchesPerIteration"],
            "membersPerLaunch": info["membersPerLaunch"], "batched": info["batched"],
            "iterations_sum": sum(iters), "iterations_max": max(iters),
            "single_ms": {"median": ms * 1e3, "min": min(ts) * 1e3, "max": max(ts) * 1e3},
            "batch_ms": {"median": mb * 1e3, "min": min(tb) * 1e3, "max": max(tb) * 1e3},
            "single_qps": B / ms, "batch_qps": B / mb, "speedup_median": ms / mb,
            # beyond the pairs' spread: the slowest batched run beats the fastest baseline run
            "faster_beyond_spread": max(tb) < min(ts),
            "single_ms_all": [t * 1e3 for t in ts], "batch_ms_all": [t * 1e3 for t in tb],
        }
        rows.append(row)
        print(f"B={B:3d}  single {ms * 1e3:8.3f} ms [{min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f}]  "
              f"batch {mb * 1e3:8.3f} ms [{min(tb) * 1e3:.3f} .. {max(tb) * 1e3:.3f}]  "
              f"x{ms / mb:.2f}  launches/iter {info['launchesPerIteration']}  "
              f"iterations sum {sum(iters)} max {max(iters)}", flush=True)
        batch.close()
    out = {"workload": "reference demo, seeds 1..B, host wall time of plan() including begin()",
           "residentGroups": i1["residentGroups"], "groupsPerMember": i1["groupsPerMember"],
           "largest_one_launch_B": largest, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"bench_batch": [{k: r[k] for k in ("B", "single_qps", "batch_qps", "speedup_median")} for r in rows]}))


if __name__ == "__main__":
    main()

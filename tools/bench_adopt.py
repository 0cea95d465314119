#!/usr/bin/env python3
"""Measure the adoption of a tree into a planner (the k_adopt_* kernels).

    python tools/bench_adopt.py [--rows 65536 1048576 16777216] [--reps 20] [--seeds 10] [--out FILE]

One JSON line per measurement on standard output; with --out FILE also into that file, which the run
starts empty (profiles/adopt/bench.jsonl is one such run).

  call     sbmp_kgmt_adopt_tree from device arrays on a planner of maxTreeSize = rows (the demo grid,
           random rows, the frontier at the last 1,024 rows), device events on the planner's stream
           round the whole call, median and best of --reps calls after --warmup calls; beside it
           sbmp_kgmt_begin on the same handle, measured the same way.  Both clear the M-row tree
           arrays and the tables and re-seed the slots; the adoption adds the scan, its read-back, the
           36-byte copy per row and the scratch allocation.
  replan   time from a blocked path to a new solution on the c5 field (systems/c5.yaml with a goal
           radius and a smaller tree), over --seeds seeds in one process: a plan, a box on the
           middle row of its solution path, then (a) recheck + replan(alive=True) + step() until the
           loop ends, against (b) the only route without the feature, begin() from the root and a
           full plan() against the new list.  Wall clock round blocking calls (recheck_ms and
           adopt_ms are route (a)'s first two calls); medians and solved counts.  No threshold is
           attached to either figure.

Before a time is printed the device's tables are compared with the host twin's
(sbmp_tree_adopt_tables against sbmp_tree_adopt_tables_host, and regions() of the adopted planner
against the twin): a difference ends the program with an error.  No GPU, no numbers.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEMO_INITIAL = (5.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0)
DEMO_GOAL = (2.0, 18.0, 0.0, 0.0, 0.0, 0.0, 0.0)
TABLES = ("R1", "R1Avail", "R1Valid", "R1Invalid", "R1Cov", "R2bits")


_out = None     # --out: the records of this run, the file truncated at the start


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    if _out is not None:
        _out.write(line + "\n")
        _out.flush()


def random_tree(rows: int):
    rng = np.random.default_rng(rows)
    state = np.zeros((rows, 4), np.float32)
    state[:, 0] = rng.uniform(0.0, 20.0, rows)
    state[:, 1] = rng.uniform(0.0, 20.0, rows)
    state[:, 2] = rng.uniform(-3.0, 3.0, rows)
    state[:, 3] = rng.uniform(-1.0, 1.0, rows)
    ctrl = np.zeros((rows, 4), np.float32)
    ctrl[:, 2] = 0.1
    ctrl[:, 3] = rng.uniform(0.0, 9.0, rows)
    parent = np.maximum(np.arange(rows, dtype=np.int64) - 1, 0).astype(np.int32) // 2
    parent[0] = -1
    return state, ctrl, parent


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--replan-tree", type=int, default=1 << 22, help="maxTreeSize of the replan measurement")
    ap.add_argument("--no-replan", action="store_true")
    ap.add_argument("--out", default=None, help="also write the records to this file (truncated first)")
    a = ap.parse_args()
    global _out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        _out = open(a.out, "w")

    from cudasbmp_amd import KGMT, DeviceBuffer, device_count, read_obstacles_csv, tree_adopt_tables
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    from cudasbmp_amd.config import workload

    if device_count() < 1:
        print("bench_adopt: no HIP device", file=sys.stderr)
        return 1
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def hip_ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with HIP error {rc}")

    def event():
        e = ctypes.c_void_p()
        hip_ok(hip.hipEventCreate(ctypes.byref(e)), "hipEventCreate")
        return e

    e0, e1 = event(), event()

    def timed(fn, stream):
        """(median, best) microseconds of fn() between two events on `stream`."""
        s = ctypes.c_void_p(stream or 0)
        times = []
        for i in range(a.warmup + a.reps):
            hip_ok(hip.hipEventRecord(e0, s), "hipEventRecord")
            fn()
            hip_ok(hip.hipEventRecord(e1, s), "hipEventRecord")
            hip_ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = ctypes.c_float()
            hip_ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
            if i >= a.warmup:
                times.append(ms.value * 1e3)
        return float(np.median(times)), float(np.min(times))

    demo = np.loadtxt(os.path.join(ROOT, "configurations", "obstacles", "obstacles.csv"), delimiter=",",
                      dtype=np.float32).reshape(-1, 4)
    d_demo = DeviceBuffer(demo)
    g7 = np.array(DEMO_GOAL, dtype=np.float32)
    i7 = np.array(DEMO_INITIAL, dtype=np.float32)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    # ---- the call, beside begin() on the same handle
    for rows in a.rows:
        state, ctrl, parent = random_tree(rows)
        frontier = max(0, rows - 1024)
        goal3 = (DEMO_GOAL[0], DEMO_GOAL[1], 0.0)
        dev = tree_adopt_tables(state, goal=goal3, frontier_from=frontier, device=True)
        twin = tree_adopt_tables(state, goal=goal3, frontier_from=frontier, device=False)
        if any(dev[k].tobytes() != twin[k].tobytes() for k in TABLES) or dev["summary"] != twin["summary"]:
            print(f"bench_adopt: device tables differ from the host twin at {rows} rows", file=sys.stderr)
            return 1
        g = KGMT(20.0, 20.0, 16, 8, 100, rows, 10, 1.0, 0.0, samplesPerIteration=262144, batchRule="fill",
                 fixGNewClear=True)
        bufs = [_Dev(x) for x in (state, ctrl, parent)]
        args = nat.TreeAdoptArgs()
        args.state, args.ctrl, args.parent = (b.ptr for b in bufs)
        args.rows, args.frontierFrom, args.depthBound, args.onDevice = rows, frontier, 0, 1
        out = nat.TreeAdopt()

        def adopt():
            nat.call("sbmp_kgmt_adopt_tree", g._h, ctypes.byref(args), vp(g7), ctypes.c_void_p(d_demo.ptr), len(demo), 1,
                     ctypes.byref(out))

        def begin():
            nat.call("sbmp_kgmt_begin", g._h, vp(i7), vp(g7), ctypes.c_void_p(d_demo.ptr), len(demo), 1)

        adopt()
        reg = g.regions()
        bits = ((twin["R2bits"][:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int32).ravel()
        if any(not np.array_equal(reg[k], twin[k]) for k in TABLES[:4]) or not np.array_equal(reg["R2Avail"], bits):
            print(f"bench_adopt: the adopted planner's tables differ from the host twin at {rows} rows", file=sys.stderr)
            return 1
        stream = g.stream()
        med, best = timed(adopt, stream)
        bmed, bbest = timed(begin, stream)
        emit({"what": "call", "rows": rows, "maxTreeSize": rows, "form": g.path_info()["form"],
              "adopt_us": round(med, 1), "adopt_best_us": round(best, 1), "begin_us": round(bmed, 1),
              "begin_best_us": round(bbest, 1), "row_bytes_copied": 72 * rows, "out_of_grid": out.outOfGrid})
        for b in bufs:
            b.close()
        g.close()

    if a.no_replan:
        return 0

    # ---- from a blocked path to a new solution, two routes
    w = workload("c5")
    field = read_obstacles_csv(w["obstacles"])
    d_field = DeviceBuffer(field)
    cfg = dict(w["planner"], goalThreshold=0.5, maxTreeSize=a.replan_tree)
    extra = dict(samplesPerIteration=w["samplesPerIteration"], batchRule=w["batchRule"], fixGNewClear=w["fixGNewClear"],
                 agent=w["agent"])
    g = KGMT(**cfg, **extra)
    recs = []
    for seed in range(1, a.seeds + 1):
        r = g.plan(w["initial"], w["goal"], d_field, len(field), seed=seed)
        rec = {"what": "replan-seed", "seed": seed, "first_plan_solved": r.goalIndex >= 0, "first_plan_rows": r.treeSize,
               "first_plan_iterations": r.iterations}
        if r.goalIndex < 0:
            emit(rec)
            recs.append(rec)
            continue
        rows, samples, _ = g.solution_path()
        mid = samples[len(rows) // 2]
        box = np.array([[mid[0] - 0.3, mid[1] - 0.3, mid[0] + 0.3, mid[1] + 0.3]], dtype=np.float32)
        new = np.concatenate([field, box]).astype(np.float32)
        d_new = DeviceBuffer(new)
        # (a) recheck, adopt what is alive, run until the loop ends
        t0 = time.perf_counter()
        _, chk = g.recheck(d_new.ptr, len(new))
        t1 = time.perf_counter()
        out = g.replan(w["goal"], d_new, len(new), seed, alive=True, frontier_from=0)
        t2 = time.perf_counter()
        while g.step(8):
            pass
        ra = g.result()
        ta = (time.perf_counter() - t0) * 1e3
        rec.update(recheck_ms=round((t1 - t0) * 1e3, 3), adopt_ms=round((t2 - t1) * 1e3, 3))
        # (b) the route without the feature
        t0 = time.perf_counter()
        rb = g.plan(w["initial"], w["goal"], d_new, len(new), seed=seed)
        tb = (time.perf_counter() - t0) * 1e3
        rec.update(alive=chk["alive"], rows=chk["rows"], goal_row_at_adoption=out["goalRow"],
                   replan_ms=round(ta, 3), replan_solved=ra.goalIndex >= 0, replan_iterations=ra.iterations - 1,
                   replan_rows=ra.treeSize, scratch_ms=round(tb, 3), scratch_solved=rb.goalIndex >= 0,
                   scratch_iterations=rb.iterations, scratch_rows=rb.treeSize)
        emit(rec)
        recs.append(rec)
        d_new.free()
    done = [x for x in recs if "replan_ms" in x]
    if done:
        emit({"what": "replan", "seeds": a.seeds, "measured": len(done), "maxTreeSize": a.replan_tree,
              "replan_ms_median": round(float(np.median([x["replan_ms"] for x in done])), 3),
              "recheck_ms_median": round(float(np.median([x["recheck_ms"] for x in done])), 3),
              "adopt_ms_median": round(float(np.median([x["adopt_ms"] for x in done])), 3),
              "scratch_ms_median": round(float(np.median([x["scratch_ms"] for x in done])), 3),
              "replan_solved": sum(x["replan_solved"] for x in done),
              "scratch_solved": sum(x["scratch_solved"] for x in done),
              "solved_at_adoption": sum(x["goal_row_at_adoption"] >= 0 for x in done)})
    return 0


if __name__ == "__main__":
    sys.exit(main())

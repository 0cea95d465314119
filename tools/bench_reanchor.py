#!/usr/bin/env python3
"""Measure the re-anchoring of a grown tree (the k_reanchor_* kernels).

    python tools/bench_reanchor.py [--rows 65536 1048576] [--chain 4096] [--reps 20] [--out FILE]

One JSON line per tree on standard output; with --out FILE also into that file, which the run
starts empty (profiles/reanchor/bench.jsonl is one such run).

  trees    the demo plan's tree and the c5 workload's tree (seed 1, their own boxes, the root
           displaced by a tracking error), random recursive trees of --rows rows (parent = any
           lower row: the deepest chain is about e ln(rows) edges, 30 at 2^16), a star of the same
           rows (two levels: what the call costs before and beside its levels) and one chain of
           --chain rows (a level a row)
  figures  sbmp_tree_reanchor_batch from device arrays with the depth bound a planner would give
           (the tree's levels) and with bound 0 (rows), beside sbmp_tree_recheck_batch of the same
           tree and boxes, the same Euler work in one launch, and the host twin; wall clock round
           the blocking calls, median and best of --reps calls after --warmup calls

Before a time is printed the device's answer (states, alive bytes, status bytes, summary) is
compared with the host twin's: a difference ends the program with an error.  No GPU, no numbers.
No threshold is attached to any figure.
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

DEMO_INITIAL = (5.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0)
DEMO_GOAL = (2.0, 18.0, 0.0, 0.0, 0.0, 0.0, 0.0)
MOVED = np.array([0.05, -0.03, 0.02, 0.0], np.float32)

_out = None


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    if _out is not None:
        _out.write(line + "\n")
        _out.flush()


def shaped_tree(rows: int, shape: str):
    """shape: random (parent = any lower row), star (parent = 0) or chain (parent = r - 1); short
    edges, so most replays stay inside the workspace."""
    rng = np.random.default_rng(rows)
    state = rng.uniform(2.0, 18.0, (rows, 4)).astype(np.float32)
    state[0] = (10.0, 10.0, 0.3, 0.5)
    ctrl = np.zeros((rows, 4), np.float32)
    ctrl[1:, 0] = rng.uniform(-5.0, 5.0, rows - 1)
    ctrl[1:, 1] = rng.uniform(-3.1, 3.1, rows - 1)
    ctrl[1:, 2] = rng.uniform(0.06, 0.12 if shape == "chain" else 0.3, rows - 1)
    r = np.arange(rows, dtype=np.int64)
    if shape == "random":
        parent = (rng.random(rows) * r).astype(np.int64)
    elif shape == "star":
        parent = np.zeros(rows, np.int64)
    else:
        parent = r - 1
    parent[0] = -1
    return state, ctrl, parent.astype(np.int32)


def planner_tree(g):
    s, p, c = g.tree()
    R = max(1, min(g.result().treeSize, len(p)))
    state = np.ascontiguousarray(s[:R, :4], np.float32)
    ctrl = np.ascontiguousarray(np.concatenate([s[:R, 4:7], c[:R, None]], axis=1), np.float32)
    return state, ctrl, np.ascontiguousarray(p[:R], np.int32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--chain", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the records to this file (truncated first)")
    a = ap.parse_args()
    global _out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        _out = open(a.out, "w")

    from cudasbmp_amd import KGMT, DeviceBuffer, device_count, read_obstacles_csv, tree_reanchor_batch
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    from cudasbmp_amd.config import workload

    if device_count() < 1:
        print("bench_reanchor: no HIP device", file=sys.stderr)
        return 1

    def timed(fn):
        """(median, best) microseconds of the blocking call fn()."""
        times = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e6)
        return round(float(np.median(times)), 1), round(float(np.min(times)), 1)

    def measure(name, state, ctrl, parent, boxes, s0, params):
        kw = dict(numDisc=params["numDisc"], agentLength=params["agentLength"], width=params["width"],
                  height=params["height"], agent=params.get("agent", "car"))
        t0 = time.perf_counter()
        twin = tree_reanchor_batch(state, ctrl, parent, s0, boxes, device=False, **kw)
        host_us = (time.perf_counter() - t0) * 1e6
        levels = twin["summary"]["levels"]
        for bound in (levels, 0):
            dev = tree_reanchor_batch(state, ctrl, parent, s0, boxes, depth_bound=bound, **kw)
            if dev["summary"] != twin["summary"] or any(dev[k].tobytes() != twin[k].tobytes()
                                                        for k in ("state", "alive", "status")):
                print(f"bench_reanchor: the device differs from the host twin on {name} (bound {bound})", file=sys.stderr)
                return False
        R = len(parent)
        bufs = [_Dev(x) for x in (state, ctrl, parent)] + ([_Dev(boxes)] if len(boxes) else [])
        outs = [_Dev(np.zeros((R, 4), np.float32)), _Dev(np.zeros(R, np.uint8))]
        args = nat.TreeRecheckArgs()
        args.state, args.ctrl, args.parent = (b.ptr for b in bufs[:3])
        args.obstacles, args.obstaclesCount = (bufs[3].ptr if len(boxes) else None), len(boxes)
        args.rows, args.agent = R, nat.SBMP_AGENT_POINT if kw["agent"] == "point" else nat.SBMP_AGENT_CAR
        args.numDisc, args.agentLength, args.width, args.height = kw["numDisc"], kw["agentLength"], kw["width"], kw["height"]
        root = np.ascontiguousarray(s0, np.float32)
        rs, cs = nat.TreeReanchor(), nat.TreeRecheck()
        status = np.zeros(R, np.uint8)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

        def reanchor():
            nat.call("sbmp_tree_reanchor_batch", ctypes.byref(args), vp(root), ctypes.c_void_p(outs[0].ptr),
                     ctypes.c_void_p(outs[1].ptr), vp(status), ctypes.byref(rs), None)

        def recheck():
            nat.call("sbmp_tree_recheck_batch", ctypes.byref(args), vp(status), ctypes.byref(cs), None)

        args.depthBound = levels
        med, best = timed(reanchor)
        cmed, cbest = timed(recheck)
        args.depthBound = 0
        med0, best0 = timed(reanchor)
        emit({"what": name, "rows": R, "boxes": len(boxes), "levels": levels, "alive": twin["summary"]["alive"],
              "blocked": twin["summary"]["blocked"], "cut": twin["summary"]["cut"],
              "reanchor_us": med, "reanchor_best_us": best, "reanchor_bound0_us": med0, "reanchor_bound0_best_us": best0,
              "recheck_us": cmed, "recheck_best_us": cbest, "host_twin_us": round(host_us, 1),
              "us_per_level": round(med / levels, 2)})
        for b in bufs + outs:
            b.close()
        return True

    demo = np.loadtxt(os.path.join(ROOT, "configurations", "obstacles", "obstacles.csv"), delimiter=",",
                      dtype=np.float32).reshape(-1, 4)
    demo_params = dict(numDisc=10, agentLength=1.0, width=20.0, height=20.0)

    g = KGMT(20.0, 20.0, 16, 8, 100, 30000, 10, 1.0, 0.5)
    g.plan(DEMO_INITIAL, DEMO_GOAL, DeviceBuffer(demo), len(demo), seed=1)
    state, ctrl, parent = planner_tree(g)
    if not measure("demo", state, ctrl, parent, demo, state[0] + MOVED, demo_params):
        return 1
    g.close()

    w = workload("c5")
    field = read_obstacles_csv(w["obstacles"])
    cfg = dict(w["planner"])
    g = KGMT(**cfg, samplesPerIteration=w["samplesPerIteration"], batchRule=w["batchRule"], fixGNewClear=w["fixGNewClear"],
             agent=w["agent"])
    g.plan(w["initial"], w["goal"], DeviceBuffer(field), len(field), seed=1)
    state, ctrl, parent = planner_tree(g)
    params = dict(numDisc=cfg["numDisc"], agentLength=cfg["agentLength"], width=cfg["width"], height=cfg["height"],
                  agent="point" if w["agent"] in (1, "point") else "car")
    if not measure("c5", state, ctrl, parent, field, state[0] + MOVED, params):
        return 1
    g.close()

    for rows in a.rows:
        for shape in ("random", "star"):
            state, ctrl, parent = shaped_tree(rows, shape)
            if not measure(f"{shape}-{rows}", state, ctrl, parent, demo, state[0], demo_params):
                return 1
    state, ctrl, parent = shaped_tree(a.chain, "chain")
    if not measure(f"chain-{a.chain}", state, ctrl, parent, demo, state[0], demo_params):
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

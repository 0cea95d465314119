#!/usr/bin/env python3
"""Measure the paths and traces of a grown tree (k_path_walk, k_tree_trace).

    python tools/bench_paths.py [--what paths trace draw] [--rows 1048576 16777216] [--reps 20]

One JSON line per measurement, also appended to profiles/paths/bench.jsonl; the first line holds
sbmp_hbm_copy_bandwidth from the same process.  Device events round the whole call on the stream
the call runs on, median and best of --reps calls after --warmup calls.

  paths   sbmp_kgmt_solution_paths (the filling call: lengths, status, rows, samples, costs) for
          Q nodes drawn from the tree, on the demo plan and on a tree grown by the c3 bench workload
          (bench.py's shape, 72 iterations), against Q consecutive sbmp_kgmt_solution_path calls in
          the same process (its sizing call left out; at most --loop-cap calls are timed and the
          rest scaled).  Q = 1 is the per-call fixed part: allocation, two waits, the copies back.
  trace   sbmp_tree_trace_batch with device output over the whole synthetic 64-level tree of
          tools/bench_recheck.py (parents one level up, consecutive) with numDisc 10, and over the
          c3-grown tree (parents scattered over the previous level); bytes per row are 4 + 16 + 16 +
          16 read and 16 numDisc + 1 written, the rate is given as a fraction of the copy rate.
  draw    the route without the kernel: KGMT.tree() plus the host twin (sbmp_tree_trace_batch_host)
          over the same rows, against KGMT.trace() of the whole tree.

Kernel times proper come from a kernel trace of this program, e.g.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_paths.py --what trace
No GPU, no numbers: the program fails without a device.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = os.path.join(ROOT, "profiles", "paths", "bench.jsonl")
QS = (1, 16, 512, 65536)
DEMO_INITIAL = (5.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0)
DEMO_GOAL = (2.0, 18.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["paths", "trace", "draw"], choices=["paths", "trace", "draw"])
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=2048)
    a = ap.parse_args()

    from cudasbmp_amd import KGMT, DeviceBuffer, device_count, read_obstacles_csv
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    from cudasbmp_amd.config import workload
    from cudasbmp_amd.kgmt import hbm_copy_bandwidth

    if device_count() < 1:
        print("bench_paths: no HIP device", file=sys.stderr)
        return 1
    lib = nat.lib()
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

    def timed(fn, stream, reps=None, warmup=None):
        """(median, best) microseconds of fn() between two events on `stream`."""
        reps = a.reps if reps is None else reps
        warmup = a.warmup if warmup is None else warmup
        s = ctypes.c_void_p(stream or 0)
        times = []
        for i in range(warmup + reps):
            hip_ok(hip.hipEventRecord(e0, s), "hipEventRecord")
            fn()
            hip_ok(hip.hipEventRecord(e1, s), "hipEventRecord")
            hip_ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = ctypes.c_float()
            hip_ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
            if i >= warmup:
                times.append(ms.value * 1e3)
        return float(np.median(times)), float(np.min(times))

    copy_gbs = hbm_copy_bandwidth()
    emit({"what": "copy", "hbm_copy_gbs": round(copy_gbs, 1)})
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def planners():
        obs = read_obstacles_csv(os.path.join(ROOT, "configurations", "obstacles", "obstacles.csv"))
        d_obs = DeviceBuffer(obs)
        demo = KGMT(20.0, 20.0, 16, 8, 100, 30000, 10, 1.0, 0.5)
        demo.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obs), seed=1)
        yield "demo", demo
        cfg = workload("c3")
        pl = dict(cfg["planner"])
        pl.update(numIterations=72, goalThreshold=0.0)
        c_obs = read_obstacles_csv(cfg["obstacles"])
        dc = DeviceBuffer(c_obs)
        c3 = KGMT(**pl, samplesPerIteration=cfg["samplesPerIteration"] or 262144, agent=cfg["agent"],
                  batchRule=cfg["batchRule"], fixGNewClear=True)
        c3.begin(cfg["initial"], cfg["goal"], dc, len(c_obs), 20240807)
        while c3.step(8):
            pass
        yield "c3-72", c3

    grown = {}
    if "paths" in a.what or "draw" in a.what or "trace" in a.what:
        for name, g in planners():
            grown[name] = g

    if "paths" in a.what:
        for name, g in grown.items():
            R = min(g.result().treeSize, g.M)
            stream = g.stream()
            rng = np.random.default_rng(11)
            for Q in QS:
                nodes = rng.integers(0, R, Q).astype(np.int32)
                total = ctypes.c_longlong()
                lengths, status = np.zeros(Q, np.int32), np.zeros(Q, np.uint8)
                nat.check(lib.sbmp_kgmt_solution_paths(g._h, vp(nodes), Q, vp(lengths), vp(status), None, None, None, 0,
                                                       ctypes.byref(total)), "sbmp_kgmt_solution_paths")
                T = total.value
                rows, samples, costs = np.zeros(T, np.int32), np.zeros((T, 7), np.float32), np.zeros(T, np.float32)

                def many():
                    nat.check(lib.sbmp_kgmt_solution_paths(g._h, vp(nodes), Q, vp(lengths), vp(status), vp(rows), vp(samples),
                                                           vp(costs), T, ctypes.byref(total)), "sbmp_kgmt_solution_paths")

                def sizing():
                    nat.check(lib.sbmp_kgmt_solution_paths(g._h, vp(nodes), Q, vp(lengths), vp(status), None, None, None, 0,
                                                           ctypes.byref(total)), "sbmp_kgmt_solution_paths")

                us, best = timed(many, stream)
                us_a, _ = timed(sizing, stream)
                n = min(Q, a.loop_cap)
                cap = int(lengths.max())
                r1, s1, c1 = np.zeros(cap, np.int32), np.zeros((cap, 7), np.float32), np.zeros(cap, np.float32)
                ln = ctypes.c_int()

                def loop():
                    for k in range(n):
                        nat.check(lib.sbmp_kgmt_solution_path(g._h, int(nodes[k]), vp(r1), vp(s1), vp(c1), cap,
                                                              ctypes.byref(ln)), "sbmp_kgmt_solution_path")

                us_loop, _ = timed(loop, stream, reps=3 if n > 64 else a.reps, warmup=1)
                emit({"what": "paths", "tree": name, "rows": R, "Q": Q, "path_rows": T,
                      "us_per_call": round(us, 1), "us_per_call_best": round(best, 1), "us_sizing_call": round(us_a, 1),
                      "us_Q_solution_path_calls": round(us_loop * Q / n, 1), "solution_path_calls_timed": n,
                      "us_per_solution_path_call": round(us_loop / n, 1)})

    def trace_stream(name, state, ctrl, parent, D=10):
        R = len(parent)
        dS, dC, dP = _Dev(state), _Dev(ctrl), _Dev(parent)
        out = ctypes.c_void_p()
        nat.call("sbmp_device_alloc", 16 * D * R + R, ctypes.byref(out))
        args = nat.TreePathsArgs()
        args.state, args.ctrl, args.parent, args.rows = dS.ptr, dC.ptr, dP.ptr, R
        args.agent, args.numDisc, args.agentLength = nat.SBMP_AGENT_CAR, D, 1.0

        def call():
            nat.check(lib.sbmp_tree_trace_batch(ctypes.byref(args), None, R, out, ctypes.c_void_p(out.value + 16 * D * R),
                                                None), "sbmp_tree_trace_batch")

        us, best = timed(call, None)
        nbytes = R * (4 + 16 + 16 + 16 + 16 * D + 1)
        status = np.zeros(R, np.uint8)
        nat.call("sbmp_device_copy_from", vp(status), ctypes.c_void_p(out.value + 16 * D * R), R)
        emit({"what": "trace", "tree": name, "rows": R, "numDisc": D, "us_per_call": round(us, 1),
              "us_per_call_best": round(best, 1), "ns_per_row": round(us * 1e3 / R, 4), "bytes": nbytes,
              "gbs": round(nbytes / us / 1e3, 1), "fraction_of_copy": round(nbytes / us / 1e3 / copy_gbs, 3),
              "free_rows": int((status == 0).sum()), "hbm_copy_gbs": round(copy_gbs, 1)})
        nat.call("sbmp_device_free", out)
        for d in (dS, dC, dP):
            d.close()

    def tree_of(g):
        from tree_recheck_model import tree_arrays
        s, p, c = g.tree()
        return tree_arrays(s, p, c, g.result().treeSize)

    if "trace" in a.what:
        from bench_recheck import synthetic_tree
        from oracle import pyoracle
        pyoracle.build()
        for R in a.rows:
            trace_stream("synthetic-64-levels", *synthetic_tree(R))
        trace_stream("c3-72", *tree_of(grown["c3-72"]))

    if "draw" in a.what:
        from cudasbmp_amd import tree_trace_batch
        for name, g in grown.items():
            us, best = timed(lambda: g.trace(), g.stream(), reps=5, warmup=1)
            t0 = time.perf_counter()
            state, ctrl, parent = tree_of(g)
            t1 = time.perf_counter()
            steps, status = tree_trace_batch(state, ctrl, parent, numDisc=g.numDisc_, agentLength=g.agentLength_, device=False)
            t2 = time.perf_counter()
            same = bool(np.array_equal(np.ascontiguousarray(steps).view(np.uint32),
                                       np.ascontiguousarray(g.trace()[0]).view(np.uint32)))
            emit({"what": "draw", "tree": name, "rows": len(parent), "us_KGMT_trace": round(us, 1),
                  "us_KGMT_trace_best": round(best, 1), "us_tree_export": round((t1 - t0) * 1e6, 1),
                  "us_host_twin": round((t2 - t1) * 1e6, 1), "same_bits": same})
            if not same:
                print(f"bench_paths: {name}: the device and the host twin differ", file=sys.stderr)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

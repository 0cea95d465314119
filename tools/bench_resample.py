#!/usr/bin/env python3
"""Measure the resample of solution paths (k_resample_clock, k_path_resample).

    python tools/bench_resample.py [--periods 0.05 0.005] [--reps 20] [--max-samples 33554432]

One JSON line per measurement, also appended to profiles/resample/bench.jsonl; the first line holds
sbmp_hbm_copy_bandwidth from the same process.  Device events round the whole call on the stream
the call runs on, median and best of --reps calls after --warmup calls, on the demo plan and on a
tree grown by the c3 bench workload (bench.py's shape, 72 iterations), for Q nodes drawn from the
tree and each period.

  resample    sbmp_kgmt_resample_paths, the filling call with host arrays (counts, status, states,
              edges, times): the walk, the clock, the kernel and the copies back
  device_out  sbmp_tree_resample_batch over a device copy of the same tree with the three sample
              arrays left on the device: the same without the copies back; its rate is 28 B per
              sample over the call, given beside the copy rate
  yardstick   the only route without the feature: KGMT.trajectories(nodes) (k_path_walk,
              k_tree_trace and their copies back) plus the host loop of the rule over the same rows
              (sbmp_tree_resample_batch_host over tree(), the export not timed), wall clock

Before a time is printed the device's bytes are compared with the host loop's: a difference ends
the program with an error.  A case with more than --max-samples samples is not run (the host loop
and the host arrays grow with it); it is printed as skipped with its total.

Kernel times proper come from a kernel trace of this program, e.g.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_resample.py --reps 5
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

OUT = os.path.join(ROOT, "profiles", "resample", "bench.jsonl")
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
    ap.add_argument("--periods", type=float, nargs="+", default=[0.05, 0.005])
    ap.add_argument("--qs", type=int, nargs="+", default=list(QS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-samples", type=int, default=1 << 25)
    a = ap.parse_args()

    from cudasbmp_amd import KGMT, DeviceBuffer, device_count, read_obstacles_csv, tree_resample_batch
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    from cudasbmp_amd.config import workload
    from cudasbmp_amd.kgmt import hbm_copy_bandwidth
    from tree_recheck_model import tree_arrays

    if device_count() < 1:
        print("bench_resample: no HIP device", file=sys.stderr)
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

    def wall(fn, reps):
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(times))

    copy_gbs = hbm_copy_bandwidth()
    emit({"what": "copy", "hbm_copy_gbs": round(copy_gbs, 1)})
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def planners():
        obs = read_obstacles_csv(os.path.join(ROOT, "configurations", "obstacles", "obstacles.csv"))
        d_obs = DeviceBuffer(obs)
        demo = KGMT(20.0, 20.0, 16, 8, 100, 30000, 10, 1.0, 0.5)
        demo.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obs), seed=1)
        yield "demo", demo, "car"
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
        yield "c3-72", c3, cfg["agent"]

    for name, g, agent in planners():
        R = min(g.result().treeSize, g.M)
        stream = g.stream()
        s, p, c = g.tree()
        state, ctrl, parent = tree_arrays(s, p, c, g.result().treeSize)
        bound = g.numIterations_ + 2
        dS, dC, dP = _Dev(state), _Dev(ctrl), _Dev(parent)
        args = nat.TreePathsArgs()
        args.state, args.ctrl, args.parent, args.rows, args.depthBound = dS.ptr, dC.ptr, dP.ptr, R, bound
        args.agent = nat.SBMP_AGENT_POINT if agent == "point" else nat.SBMP_AGENT_CAR
        args.numDisc, args.agentLength = g.numDisc_, g.agentLength_
        rng = np.random.default_rng(11)
        for Q in a.qs:
            nodes = rng.integers(0, R, Q).astype(np.int32)
            for period in a.periods:
                total = ctypes.c_longlong()
                counts, status = np.zeros(Q, np.int32), np.zeros(Q, np.uint8)
                per = ctypes.c_double(period)
                nat.check(lib.sbmp_kgmt_resample_paths(g._h, vp(nodes), Q, per, vp(counts), vp(status), None, None, None,
                                                       0, ctypes.byref(total)), "sbmp_kgmt_resample_paths")
                T = total.value
                base = {"tree": name, "rows": R, "Q": Q, "period": period, "samples": T}
                if T > a.max_samples:
                    emit(dict(base, what="skipped", reason=f"more than --max-samples {a.max_samples}"))
                    continue
                states, edges, times = np.zeros((T, 4), np.float32), np.zeros(T, np.int32), np.zeros(T, np.float64)

                def fill():
                    nat.check(lib.sbmp_kgmt_resample_paths(g._h, vp(nodes), Q, per, vp(counts), vp(status), vp(states),
                                                           vp(edges), vp(times), T, ctypes.byref(total)),
                              "sbmp_kgmt_resample_paths")

                def sizing():
                    nat.check(lib.sbmp_kgmt_resample_paths(g._h, vp(nodes), Q, per, vp(counts), vp(status), None, None,
                                                           None, 0, ctypes.byref(total)), "sbmp_kgmt_resample_paths")

                # the yardstick's two halves, and the comparison of the bytes
                twin = {}

                def host_loop():
                    twin.update(tree_resample_batch(state, ctrl, parent, nodes, period, numDisc=g.numDisc_,
                                                    agentLength=g.agentLength_, agent=agent, depthBound=bound,
                                                    device=False))

                slow = T > (1 << 21)
                us_host = wall(host_loop, 1 if slow else 3)
                fill()
                same = (states.tobytes() == twin["states"].tobytes() and edges.tobytes() == twin["edges"].tobytes()
                        and times.tobytes() == twin["times"].tobytes() and counts.tobytes() == twin["counts"].tobytes())
                if not same:
                    print(f"bench_resample: {name} Q {Q} period {period}: the device and the host loop differ",
                          file=sys.stderr)
                    return 1
                reps = max(3, a.reps // 4) if slow else a.reps
                us, best = timed(fill, stream, reps=reps)
                us_size, _ = timed(sizing, stream, reps=reps)
                us_traj = wall(lambda: g.trajectories(nodes), 3 if slow else 5)

                out = ctypes.c_void_p()
                nat.call("sbmp_device_alloc", max(T, 1) * 28, ctypes.byref(out))

                def device_out():
                    nat.check(lib.sbmp_tree_resample_batch(ctypes.byref(args), vp(nodes), Q, per, vp(counts), vp(status), out,
                                                           ctypes.c_void_p(out.value + 24 * T), ctypes.c_void_p(out.value + 16 * T),
                                                           T, ctypes.byref(total), None), "sbmp_tree_resample_batch")

                us_dev, best_dev = timed(device_out, None, reps=reps)
                nat.call("sbmp_device_free", out)
                emit(dict(base, what="resample", same_bytes=True, us_per_call=round(us, 1), us_per_call_best=round(best, 1),
                          us_sizing_call=round(us_size, 1), us_device_out=round(us_dev, 1),
                          us_device_out_best=round(best_dev, 1), gbs_written_device_out=round(28 * T / us_dev / 1e3, 2),
                          hbm_copy_gbs=round(copy_gbs, 1), us_yardstick=round(us_traj + us_host, 1),
                          us_trajectories=round(us_traj, 1), us_host_loop=round(us_host, 1)))
        for d in (dS, dC, dP):
            d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Measure the tree extraction, prune and re-root (the k_extract_* kernels).

    python tools/bench_extract.py [--rows 65536 1048576 16777216] [--reps 20] [--route-rows 1048576]

One JSON line per measurement, also appended to profiles/extract/bench.jsonl; the first line holds
sbmp_hbm_copy_bandwidth from the same process.  Device events round the whole call on the stream
the call runs on, median and best of --reps calls after --warmup calls.

  step     sbmp_tree_extract_batch with every output in device memory over §5.9's synthetic
           64-level tree (tools/bench_recheck.py), depthBound 65: with all rows kept, with the alive
           mask the device's re-check leaves for each of §5.9's three lists (demo, 600, c5), and
           re-rooted at the first row of depth 8 with all rows kept
  planner  sbmp_kgmt_extract_tree, the filling call with host arrays, on the demo plan and on a tree
           grown by the c3 bench workload (72 iterations)

must_move_bytes is what the kernels cannot avoid: per row the parent word, the keep byte when there
is a mask and the newRow word; per member 32 bytes read and 40 written.  gbs_must_move is that over
the call's time, beside the copy rate of the same process; the call also allocates its scratch,
which is what limits it.

The yardstick is the only route without the feature: the export of the whole tree to the host
(KGMT.tree(), or the same bytes copied from the device arrays) plus the numpy model of
tests/tree_extract_model.py, wall clock in the same process.  Above --route-rows rows it runs on a
prefix of that many rows (a prefix of a tree is a tree) and is scaled linearly: `yardstick` says
"full" or "scaled from N rows".

Before a time is printed the device's bytes are compared with the host twin's: a difference ends
the program with an error.  Kernel times proper come from a kernel trace of this program, e.g.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_extract.py --reps 5
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

OUT = os.path.join(ROOT, "profiles", "extract", "bench.jsonl")
DEMO_INITIAL = (5.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0)
DEMO_GOAL = (2.0, 18.0, 0.0, 0.0, 0.0, 0.0, 0.0)
NAMES = ("state", "ctrl", "parent", "origin", "newRow")


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def must_move(rows, kept, masked):
    return rows * (4 + (1 if masked else 0) + 4) + kept * (32 + 40)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--lists", nargs="+", default=["demo", "600", "c5"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-rows", type=int, default=1 << 20)
    ap.add_argument("--no-planner", action="store_true")
    a = ap.parse_args()

    from bench_recheck import LEVELS, PARAMS, box_list, synthetic_tree
    from cudasbmp_amd import KGMT, DeviceBuffer, device_count, read_obstacles_csv, tree_extract_batch
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    from cudasbmp_amd.config import workload
    from cudasbmp_amd.kgmt import hbm_copy_bandwidth
    from oracle import pyoracle
    from tree_extract_model import extract_model
    from tree_recheck_model import tree_arrays

    if device_count() < 1:
        print("bench_extract: no HIP device", file=sys.stderr)
        return 1
    pyoracle.build()
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

    copy_gbs = hbm_copy_bandwidth()
    emit({"what": "copy", "hbm_copy_gbs": round(copy_gbs, 1)})
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def same_bytes(got, want, kept):
        return all(np.ascontiguousarray(got[k][:kept] if k != "newRow" else got[k]).tobytes()
                   == np.ascontiguousarray(want[k]).tobytes() for k in NAMES)

    def yardstick(export, n, root, keep):
        """(microseconds, label): export(n) -> (state, ctrl, parent) on the host, then the model."""
        t0 = time.perf_counter()
        st, ct, pa = export(n)
        extract_model(st, ct, pa, min(root, n - 1), None if keep is None else keep[:n])
        return (time.perf_counter() - t0) * 1e6

    # ---------------------------------------------------------------- step level
    for R in a.rows:
        state, ctrl, parent = synthetic_tree(R)
        dS, dC, dP = _Dev(state), _Dev(ctrl), _Dev(parent)
        outs = {"state": _Dev(np.zeros((R, 4), np.float32)), "ctrl": _Dev(np.zeros((R, 4), np.float32)),
                "parent": _Dev(np.zeros(R, np.int32)), "origin": _Dev(np.zeros(R, np.int32)),
                "newRow": _Dev(np.zeros(R, np.int32))}
        args = nat.TreeExtractArgs()
        args.state, args.ctrl, args.parent, args.rows, args.depthBound = dS.ptr, dC.ptr, dP.ptr, R, LEVELS + 1
        masks = [("all", None, 0)]
        for name in a.lists:                       # the alive mask the device's own re-check leaves
            boxes = box_list(name)
            dB = _Dev(boxes)
            ra = nat.TreeRecheckArgs()
            ra.state, ra.ctrl, ra.parent = dS.ptr, dC.ptr, dP.ptr
            ra.rows, ra.depthBound, ra.agent, ra.numDisc = R, LEVELS + 1, nat.SBMP_AGENT_CAR, PARAMS["numDisc"]
            ra.agentLength, ra.width, ra.height = PARAMS["agentLength"], PARAMS["width"], PARAMS["height"]
            ra.obstacles, ra.obstaclesCount = dB.ptr, len(boxes)
            status = np.zeros(R, np.uint8)
            rs = nat.TreeRecheck()
            nat.check(lib.sbmp_tree_recheck_batch(ctypes.byref(ra), vp(status), ctypes.byref(rs), None), "sbmp_tree_recheck_batch")
            dB.close()
            masks.append((f"alive-{name}", (status == 0).astype(np.uint8), 0))
        d8 = min(R - 1, 1 + 7 * max(1, (R - 1) // LEVELS))   # the first row of level 8: 8 edges below the root
        masks.append(("reroot-depth-8", None, d8))

        def export(n):
            got = []
            for src, shape, dt in ((dS, (n, 4), np.float32), (dC, (n, 4), np.float32), (dP, (n,), np.int32)):
                tmp = np.empty(shape, dt)
                nat.call("sbmp_device_copy_from", vp(tmp), ctypes.c_void_p(src.ptr), tmp.nbytes)
                got.append(tmp)
            return got

        for label, keep, root in masks:
            dK = _Dev(keep) if keep is not None else None
            s = nat.TreeExtract()

            def call():
                nat.check(lib.sbmp_tree_extract_batch(ctypes.byref(args), root, ctypes.c_void_p(dK.ptr) if dK else None,
                                                      *(ctypes.c_void_p(outs[k].ptr) for k in NAMES), R, ctypes.byref(s),
                                                      None), "sbmp_tree_extract_batch")

            call()
            twin = tree_extract_batch(state, ctrl, parent, root=root, keep=keep, device=False)
            got = {k: outs[k].get() for k in NAMES}
            if s.kept != twin["summary"]["kept"] or not same_bytes(got, twin, s.kept):
                print(f"bench_extract: rows {R} {label}: the device and the host twin differ", file=sys.stderr)
                return 1
            del got, twin
            us, best = timed(call, None)
            n = min(R, a.route_rows)
            us_yard = yardstick(export, n, root, keep) * (R / n)
            mm = must_move(R, s.kept, keep is not None)
            emit({"what": "step", "rows": R, "case": label, "root": root, "kept": s.kept, "masked": s.masked,
                  "detached": s.detached, "below": s.below, "same_bytes": True, "us_per_call": round(us, 1),
                  "us_per_call_best": round(best, 1), "ns_per_row": round(us * 1e3 / R, 3), "must_move_bytes": mm,
                  "gbs_must_move": round(mm / us / 1e3, 1), "hbm_copy_gbs": round(copy_gbs, 1),
                  "us_yardstick": round(us_yard, 1), "yardstick": "full" if n == R else f"scaled from {n} rows"})
            if dK:
                dK.close()
        for d in [dS, dC, dP] + list(outs.values()):
            d.close()
    if a.no_planner:
        return 0

    # ---------------------------------------------------------------- planner level
    def planners():
        obs = read_obstacles_csv(os.path.join(ROOT, "configurations", "obstacles", "obstacles.csv"))
        d_obs = DeviceBuffer(obs)
        demo = KGMT(20.0, 20.0, 16, 8, 100, 30000, 10, 1.0, 0.5)
        demo.plan(DEMO_INITIAL, DEMO_GOAL, d_obs, len(obs), seed=1)
        yield "demo", demo, obs
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
        yield "c3-72", c3, c_obs

    for name, g, obs in planners():
        R = min(g.result().treeSize, g.M)
        stream = g.stream()
        g.recheck(obs)                                     # a mask for the alive form (the plan's own list)
        for label, root, alive in (("whole", 0, 0), ("alive", 0, 1), ("reroot", R // 7, 0)):
            s = nat.TreeExtract()
            nat.check(lib.sbmp_kgmt_extract_tree(g._h, root, alive, None, None, None, None, None, 0, ctypes.byref(s)),
                      "sbmp_kgmt_extract_tree")
            K = max(1, s.kept)
            o = {"state": np.zeros((K, 4), np.float32), "ctrl": np.zeros((K, 4), np.float32), "parent": np.zeros(K, np.int32),
                 "origin": np.zeros(K, np.int32), "newRow": np.zeros(R, np.int32)}

            def fill():
                nat.check(lib.sbmp_kgmt_extract_tree(g._h, root, alive, *(vp(o[k]) for k in NAMES), K, ctypes.byref(s)),
                          "sbmp_kgmt_extract_tree")

            def sizing():
                nat.check(lib.sbmp_kgmt_extract_tree(g._h, root, alive, None, None, None, None, None, 0, ctypes.byref(s)),
                          "sbmp_kgmt_extract_tree")

            keep = None
            if alive:
                keep = (g.recheck(obs)[0] == 0).astype(np.uint8)

            def route():
                sm, p, c = g.tree()
                st, ct, pa = tree_arrays(sm, p, c, g.result().treeSize)
                return extract_model(st, ct, pa, root, keep)

            t0 = time.perf_counter()
            want = route()
            us_yard = (time.perf_counter() - t0) * 1e6
            fill()
            if s.kept != want["summary"]["kept"] or not same_bytes(o, want, s.kept):
                print(f"bench_extract: {name} {label}: the device and the model differ", file=sys.stderr)
                return 1
            us, best = timed(fill, stream)
            us_size, _ = timed(sizing, stream)
            mm = must_move(R, s.kept, bool(alive))
            emit({"what": "planner", "tree": name, "rows": R, "case": label, "root": root, "kept": s.kept, "same_bytes": True,
                  "us_per_call": round(us, 1), "us_per_call_best": round(best, 1), "us_sizing_call": round(us_size, 1),
                  "must_move_bytes": mm, "gbs_must_move": round(mm / us / 1e3, 2), "hbm_copy_gbs": round(copy_gbs, 1),
                  "us_yardstick": round(us_yard, 1), "yardstick": "full"})
    return 0


if __name__ == "__main__":
    sys.exit(main())

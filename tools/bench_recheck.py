#!/usr/bin/env python3
"""Measure the tree re-check (k_tree_recheck + k_tree_alive) on synthetic trees.

    python tools/bench_recheck.py [--rows 65536 1048576 16777216] [--lists demo 600 c5] [--reps 20]

The tree: row 0 the root at (10, 10), then levels of `width` = (rows - 1) / 64 rows; a row of
level 1 hangs below the root, a row of a deeper level below the row `width` before it.  Every row
is what the CPU oracle's replay makes of its parent and seeded controls with no boxes (a row that
leaves the workspace is stored where it stopped), so against an empty list every row replays bit
for bit; the lists then block what they block.  For every (rows, list) pair one JSON line:

  us_per_call        sbmp_tree_recheck_batch as its caller sees it on the stream: device events
                     round the whole call (the list's device copy, NaN scan and grid index, the
                     scratch allocation, k_tree_recheck, the k_tree_alive passes, the summary's copy
                     back and the wait), median and best of --reps calls after --warmup calls.
                     depthBound = 65, so 7 pointer-jumping passes.  No status bytes are copied back.
  ns_per_row         us_per_call / rows
  summary            the call's counts
  replay_route_ms    the route without the kernels: the device-to-host copy of the export (rows x 7
                     floats, parents, costs), oracle.pyoracle.replay on 16 threads, and an ascending
                     walk for `alive`.  Timed on at most --route-rows rows and scaled linearly to
                     `rows` (replay_route_rows says on how many it ran).
  matches_model      the status bytes of one more call equal the model's (only where the route ran
                     on all rows)

Kernel times proper come from a kernel trace of this program, e.g.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_recheck.py ...
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

LEVELS = 64
PARAMS = dict(numDisc=10, agentLength=1.0, width=20.0, height=20.0, agent="car")


def synthetic_tree(rows: int):
    from tree_recheck_model import replay_rows
    width = max(1, (rows - 1) // LEVELS)
    rng = np.random.default_rng(rows)
    state = np.zeros((rows, 4), np.float32)
    ctrl = np.zeros((rows, 4), np.float32)
    state[0] = (10.0, 10.0, 0.0, 0.5)
    ctrl[1:, 0] = rng.uniform(-1.0, 1.0, rows - 1)
    ctrl[1:, 1] = rng.uniform(-0.5, 0.5, rows - 1)
    ctrl[1:, 2] = rng.uniform(0.06, 0.2, rows - 1)
    r = np.arange(rows, dtype=np.int64)
    parent = np.where(r <= width, 0, r - width).astype(np.int32)
    parent[0] = -1
    none = np.zeros((0, 4), np.float32)
    for lo in range(1, rows, width):
        hi = min(rows, lo + width)
        par = state[parent[lo:hi]]
        # replay_rows takes a tree: give it the parents as rows 0 .. n - 1 and the level as their children
        n = hi - lo
        st = np.concatenate([par, np.zeros((n, 4), np.float32)])
        ct = np.concatenate([np.zeros((n, 4), np.float32), ctrl[lo:hi]])
        pa = np.concatenate([np.full(n, -1, np.int32), np.arange(n, dtype=np.int32)])
        _, out, _ = replay_rows(st, ct, pa, none, threads=16, **PARAMS)
        state[lo:hi] = out[n:]
        ctrl[lo:hi, 3] = ctrl[parent[lo:hi], 3] + ctrl[lo:hi, 2]
    return state, ctrl, parent


def box_list(name: str) -> np.ndarray:
    from scenarios import demo_boxes, random_boxes
    if name == "demo":
        return demo_boxes()
    if name == "c5":
        return np.loadtxt(os.path.join(ROOT, "configurations", "obstacles", "obstacles_c5.csv"), delimiter=",",
                          dtype=np.float32).reshape(-1, 4)
    return random_boxes(int(name), 20.0, 20.0, 7, 0.3, 0.8, root=(10.0, 10.0, 0.0, 0.0))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--lists", nargs="+", default=["demo", "600", "c5"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-rows", type=int, default=1 << 18)
    a = ap.parse_args()

    from cudasbmp_amd import _native as nat
    from cudasbmp_amd import device_count
    from cudasbmp_amd.batch import _Dev
    from oracle import pyoracle
    from tree_recheck_model import recheck_model, summary_of

    if device_count() < 1:
        print("bench_recheck: no HIP device", file=sys.stderr)
        return 1
    pyoracle.build()
    lib = nat.lib()
    try:   # events on the default stream, where the call runs
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

    for R in a.rows:
        state, ctrl, parent = synthetic_tree(R)
        dS, dC, dP = _Dev(state), _Dev(ctrl), _Dev(parent)
        for name in a.lists:
            boxes = box_list(name)
            dB = _Dev(boxes)
            args = nat.TreeRecheckArgs()
            args.state, args.ctrl, args.parent = dS.ptr, dC.ptr, dP.ptr
            args.rows, args.depthBound, args.agent, args.numDisc = R, LEVELS + 1, nat.SBMP_AGENT_CAR, PARAMS["numDisc"]
            args.agentLength, args.width, args.height = PARAMS["agentLength"], PARAMS["width"], PARAMS["height"]
            args.obstacles, args.obstaclesCount = dB.ptr, len(boxes)
            out = nat.TreeRecheck()

            def call(status=None):
                nat.check(lib.sbmp_tree_recheck_batch(ctypes.byref(args), status, ctypes.byref(out), None),
                          "sbmp_tree_recheck_batch")

            times = []
            for i in range(a.warmup + a.reps):
                hip_ok(hip.hipEventRecord(e0, None), "hipEventRecord")
                call()
                hip_ok(hip.hipEventRecord(e1, None), "hipEventRecord")
                hip_ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
                ms = ctypes.c_float()
                hip_ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
                if i >= a.warmup:
                    times.append(ms.value * 1e3)
            us_med, us_min = float(np.median(times)), float(np.min(times))
            summary = {k: getattr(out, k) for k, _ in nat.TreeRecheck._fields_}

            # the route without the kernels, on a prefix of the tree (a prefix of a tree is a tree)
            n = min(R, a.route_rows)
            t0 = time.perf_counter()
            # the export's bytes: rows x (7 floats of samples, a parent, a cost), as KGMT.tree() copies them
            hs = np.empty((n, 7), np.float32)
            hp = np.empty(n, np.int32)
            hc = np.empty(n, np.float32)
            for dst, src in ((hs[:, :4], dS), (hs[:, 4:], dC), (hp, dP), (hc, dC)):
                tmp = np.empty(dst.shape, dst.dtype)
                nat.call("sbmp_device_copy_from", tmp.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(src.ptr), tmp.nbytes)
            hs[:, :4], hs[:, 4:], hp[:], hc[:] = state[:n], ctrl[:n, :3], parent[:n], ctrl[:n, 3]
            copy_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            st = np.ascontiguousarray(hs[:, :4])
            ct = np.ascontiguousarray(np.concatenate([hs[:, 4:7], hc[:, None]], axis=1))
            want, wsum, _ = recheck_model(st, ct, hp, boxes, threads=16, **PARAMS)
            model_ms = (time.perf_counter() - t0) * 1e3
            matches = None
            if n == R:
                status = np.zeros(R, np.uint8)
                call(status.ctypes.data_as(ctypes.c_void_p))
                matches = bool(np.array_equal(status, want)) and summary_of(status) == wsum
                if not matches:
                    print(f"bench_recheck: rows {R} list {name}: the device and the model differ", file=sys.stderr)
                    return 1
            dB.close()
            print(json.dumps({
                "rows": R, "list": name, "boxes": len(boxes), "reps": a.reps,
                "us_per_call": round(us_med, 2), "us_per_call_best": round(us_min, 2),
                "ns_per_row": round(us_med * 1e3 / R, 3), "summary": summary,
                "replay_route_ms": round((copy_ms + model_ms) * (R / n), 1), "replay_route_rows": n,
                "export_copy_ms": round(copy_ms * (R / n), 1), "matches_model": matches,
            }), flush=True)
        for d in (dS, dC, dP):
            d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Measure k_tree_query (goal queries against tree rows) on synthetic rows.

    python tools/bench_query.py [--rows 1048576 16777216] [--goals 1 8 64 512] [--reps 20]

For every (rows, goals) pair it prints one JSON line:

  us_per_call        sbmp_tree_query_batch as its caller sees it on the stream: device events
                     round the whole call (thresholds on the host, the accumulators' allocation,
                     the init kernel, one k_tree_query launch per 16 goals, the copy of the
                     answers back and the wait for it), median and best of --reps calls after
                     --warmup calls.  A device-side delay queued first holds the stream while the
                     host prepares and enqueues, so the launches run back to back.
  passes             k_tree_query launches per call (one pass over the rows each)
  stream_GBs         rows x 16 B x passes / us_per_call: the treeState bytes streamed per second
  pairs_per_s        goals x rows / us_per_call
  hbm_copy_GBs       sbmp_hbm_copy_bandwidth of this device, measured in the same process
  numpy_route_ms     what the same answers cost without the kernel: the device-to-host copy of
                     the export (rows x 7 floats of samples, rows floats of costs, as KGMT.tree())
                     plus the numpy model over it.  The model is timed on at most --model-goals
                     goals and scaled to the goal count (it is linear in it).

Kernel times proper (without the call's host side) come from a kernel trace of this program,
e.g.  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_query.py ...

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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--goals", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--model-goals", type=int, default=4)
    ap.add_argument("--hbm-bytes", type=int, default=1 << 30)
    a = ap.parse_args()

    import torch

    from cudasbmp_amd import _native as nat
    from cudasbmp_amd import device_count
    from cudasbmp_amd.kgmt import hbm_copy_bandwidth
    from cudasbmp_amd.tree_query import ANSWER_DTYPE, answers_dict
    from tree_query_model import assert_same_answers, query_model

    if device_count() < 1 or not torch.cuda.is_available():
        print("bench_query: no HIP device", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    hbm = hbm_copy_bandwidth(a.hbm_bytes, 5)
    stream = torch.cuda.Stream(device=dev)
    sptr = ctypes.c_void_p(stream.cuda_stream)
    lib = nat.lib()

    for R in a.rows:
        gen = torch.Generator(device=dev).manual_seed(R)
        # rows over the demo's 20 x 20 workspace, costs up to 30: the planner's tree layout
        state = torch.rand((R, 4), generator=gen, device=dev, dtype=torch.float32) * 20.0
        ctrl = torch.rand((R, 4), generator=gen, device=dev, dtype=torch.float32) * 30.0
        samples = torch.cat([state, ctrl[:, :3]], dim=1).contiguous()   # the export layout, rows x 7
        costs = ctrl[:, 3].contiguous()
        torch.cuda.synchronize()
        for Q in a.goals:
            rng = np.random.default_rng(Q)
            goals = np.concatenate([rng.uniform(0.0, 20.0, size=(Q, 2)), np.full((Q, 1), a.radius)],
                                   axis=1).astype(np.float32)
            out = np.zeros(Q, dtype=ANSWER_DTYPE)

            def call():
                nat.check(lib.sbmp_tree_query_batch(ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(ctrl.data_ptr()),
                                                    R, goals.ctypes.data_as(ctypes.c_void_p), Q,
                                                    out.ctypes.data_as(ctypes.c_void_p), sptr), "sbmp_tree_query_batch")

            times = []
            for i in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    torch.cuda._sleep(2_000_000)   # ~1 ms: the host enqueues the whole call behind it
                    e0.record(stream)
                    call()
                    e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    times.append(e0.elapsed_time(e1) * 1e3)
            us_med, us_min = float(np.median(times)), float(np.min(times))
            passes = (Q + 15) // 16

            # the route without the kernel: export to the host, then numpy
            t0 = time.perf_counter()
            hs, hc = samples.cpu().numpy(), costs.cpu().numpy()
            copy_ms = (time.perf_counter() - t0) * 1e3
            qm = min(Q, a.model_goals)
            t0 = time.perf_counter()
            model = query_model(hs[:, 0], hs[:, 1], hc, goals[:qm])
            model_ms = (time.perf_counter() - t0) * 1e3 * (Q / qm)
            assert_same_answers({k: v[:qm] for k, v in answers_dict(out).items()}, model, label=f"rows {R} goals {Q}")

            print(json.dumps({
                "rows": R, "goals": Q, "passes": passes, "reps": a.reps,
                "us_per_call": round(us_med, 2), "us_per_call_best": round(us_min, 2),
                "stream_GBs": round(R * 16.0 * passes / us_med / 1e3, 1),
                "pairs_per_s": float(f"{Q * R / (us_med * 1e-6):.4g}"),
                "hbm_copy_GBs": round(hbm, 1),
                "numpy_route_ms": round(copy_ms + model_ms, 1), "export_copy_ms": round(copy_ms, 1),
                "model_goals_timed": qm, "answers_match_model": True,
            }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

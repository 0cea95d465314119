"""The fold of the R2 key log into R2Valid / R2Invalid over caller arrays (the rule:
include/sbmp/r2_fold.h).

    fold_r2_info    the window, the keys per fold workgroup, the largest nR2 and nranks, and the
                    launcher's split of a log row of logSlots keys (sbmp_fold_r2_info, host-only)
    fold_r2_batch   k_fold_r2 through the planner's own launcher on the GPU (sbmp_fold_r2_batch),
                    or, with device=False, the rule's host loop (sbmp_fold_r2_batch_host)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat


def fold_r2_info(logSlots: int) -> dict:
    info = nat.FoldInfo()
    nat.call("sbmp_fold_r2_info", int(logSlots), ctypes.byref(info))
    return {n: getattr(info, n) for n, _ in nat.FoldInfo._fields_}


def fold_r2_batch(ring, S, executed, tFirst, nR2, *, rank=0, nranks=1, R2Valid=None, R2Invalid=None, device=True,
                  repeat=1):
    """ring (window, logSlots) uint16 keys; S, executed: one int per iteration tFirst, tFirst + 1,
    ...; R2Valid / R2Invalid: (nR2,) int32 prior contents (zeros if None), not modified.  Returns
    the two tables after `repeat` folds of the same iterations (each adds to the last)."""
    from .batch import _Dev
    ring = np.ascontiguousarray(ring, dtype=np.uint16)
    if ring.ndim != 2:
        raise ValueError("ring must be (window, logSlots)")
    if ring.shape[0] != fold_r2_info(ring.shape[1])["window"]:
        raise ValueError("ring must hold one row per iteration of the window")
    S = np.ascontiguousarray(S, dtype=np.int32).reshape(-1)
    ex = np.ascontiguousarray(executed, dtype=np.int32).reshape(-1)
    if len(S) != len(ex):
        raise ValueError("S and executed must have one entry per iteration")
    tables = [np.zeros(nR2, dtype=np.int32) if t is None else np.array(t, dtype=np.int32).reshape(-1).copy()
              for t in (R2Valid, R2Invalid)]
    if any(len(t) != nR2 for t in tables):
        raise ValueError("R2Valid and R2Invalid must hold nR2 ints")
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = (hp(S), hp(ex), int(tFirst), int(tFirst) + len(S) - 1, ring.shape[1], int(nR2), int(rank), int(nranks))
    if not device:
        for _ in range(repeat):
            nat.call("sbmp_fold_r2_batch_host", hp(ring), *args, hp(tables[0]), hp(tables[1]))
        return tables[0], tables[1]
    devs = []
    try:
        for a in (ring, tables[0], tables[1]):
            devs.append(_Dev(a))
        dp = [ctypes.c_void_p(d.ptr) for d in devs]
        for _ in range(repeat):
            nat.call("sbmp_fold_r2_batch", dp[0], *args, dp[1], dp[2], None)
        return devs[1].get(), devs[2].get()
    finally:
        for d in devs:
            d.close()

"""KGMTBatch: several independent queries on one map, planned together on one GPU.

No reference counterpart (the reference plans one query per KGMT object).  A batch holds
`count` planners with one parameter set on one stream; the members take their own initial
states, goals and seeds and share the obstacle list.  While they run the one-launch form,
one k_step_batch launch per iteration advances as many members as the device holds at
once (sbmp_kgmt_batch_* in include/sbmp/sbmp.h).  Every member computes
exactly what KGMT.plan computes for its query.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence

import numpy as np

from . import _native as nat
from .kgmt import KGMT, device_ptr, _kgmt_params

SBMP_ERR_UNSUPPORTED = 6


def batch_pack(groups_per_member: Sequence[int], resident_groups: int):
    """The packing rule alone (sbmp_batch_pack, host-only): (launch of each member, or -1 for
    a member that does not fit alone; number of launches)."""
    g = np.ascontiguousarray(groups_per_member, dtype=np.int32)
    out = np.zeros(max(1, len(g)), dtype=np.int32)
    n = ctypes.c_int()
    nat.call("sbmp_batch_pack", g.ctypes.data_as(ctypes.c_void_p) if len(g) else None, len(g), int(resident_groups),
             out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
    return out[: len(g)].tolist(), n.value


class _Member(KGMT):
    """Member i of a batch: every read method of KGMT on a handle the batch owns.  Planning
    calls on it (plan, begin, step, enqueue) fail with SBMP_ERR_STATE."""

    def __init__(self, batch: "KGMTBatch", i: int):   # no KGMT.__init__: the handle is borrowed
        h = ctypes.c_void_p()
        nat.call("sbmp_kgmt_batch_member", batch._h, i, ctypes.byref(h))
        self._h = h
        self._batch = batch   # the batch owns the planner: keep it alive
        self._coll = None
        self._set_reference_fields(batch.width_, batch.height_, batch.N_, batch.n_, batch.numIterations_,
                                   batch.maxTreeSize_, batch.numDisc_, batch.agentLength_, batch.goalThreshold_)

    def close(self):
        self._h = ctypes.c_void_p()


class KGMTBatch:
    """`count` KGMT planners with one parameter set, planned together (KGMT's constructor arguments)."""

    def __init__(self, count: int, width: float, height: float, N: int, n: int, numIterations: int,
                 maxTreeSize: int, numDisc: int, agentLength: float, goalThreshold: float, *,
                 samplesPerIteration: int = 0, agent: str = "car", fixGNewClear: bool = False, device: int = 0,
                 profileKernels: bool = False, batchRule: str = "reference", _sharded=None, _local_group: int = 0,
                 _host_sharded=None):
        self._h = ctypes.c_void_p()
        if _sharded is not None or _local_group or _host_sharded is not None:
            raise nat.SbmpError(SBMP_ERR_UNSUPPORTED, "KGMTBatch",
                                "sharded and local-group planners are not supported in a batch")
        p = _kgmt_params(width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength, goalThreshold,
                        samplesPerIteration, agent, fixGNewClear, device, profileKernels, batchRule)
        self._params = p
        self.count = int(count)
        h = ctypes.c_void_p()
        nat.call("sbmp_kgmt_batch_create", ctypes.byref(p), self.count, ctypes.byref(h))
        self._h = h
        KGMT._set_reference_fields(self, width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength,
                                   goalThreshold)
        self._members = [_Member(self, i) for i in range(self.count)]

    @classmethod
    def from_params(cls, count: int, **kw) -> "KGMTBatch":
        base = dict(width=20.0, height=20.0, N=16, n=8, numIterations=100, maxTreeSize=30000, numDisc=10,
                    agentLength=1.0, goalThreshold=0.5)
        base.update(kw)
        return cls(count, **base)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            for m in getattr(self, "_members", []):
                m.close()
            nat.call("sbmp_kgmt_batch_destroy", self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return self.count

    def __getitem__(self, i: int) -> KGMT:
        return self._members[i]

    def _inputs(self, initials, goals, seeds):
        def rows(v):
            a = np.zeros((self.count, 7), dtype=np.float32)
            v = [np.asarray(r, dtype=np.float32).ravel() for r in v]
            if len(v) != self.count:
                raise ValueError(f"expected {self.count} rows, got {len(v)}")
            for k, r in enumerate(v):
                a[k, : len(r)] = r
            return a
        s = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        if len(s) != self.count:
            raise ValueError(f"expected {self.count} seeds, got {len(s)}")
        return rows(initials), rows(goals), s

    # ---------------------------------------------------------------- planning
    def plan(self, initials, goals, d_obstacles, obstaclesCount: int, seeds) -> List[nat.PlanResult]:
        """Every member's KGMT::plan, together; blocking.  A member's wallMs runs to its own end."""
        i, g, s = self._inputs(initials, goals, seeds)
        res = (nat.PlanResult * self.count)()
        self._obs_keepalive = d_obstacles
        nat.call("sbmp_kgmt_batch_plan", self._h, i.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p),
                 ctypes.c_void_p(device_ptr(d_obstacles)), obstaclesCount, s.ctypes.data_as(ctypes.c_void_p),
                 ctypes.cast(res, ctypes.c_void_p))
        out = []
        for k in range(self.count):
            r = nat.PlanResult.from_buffer_copy(res[k])
            self._members[k]._absorb(r)
            out.append(r)
        return out

    def begin(self, initials, goals, d_obstacles, obstaclesCount: int, seeds) -> None:
        i, g, s = self._inputs(initials, goals, seeds)
        self._obs_keepalive = d_obstacles
        nat.call("sbmp_kgmt_batch_begin", self._h, i.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p),
                 ctypes.c_void_p(device_ptr(d_obstacles)), obstaclesCount, s.ctypes.data_as(ctypes.c_void_p))

    def step(self, iterations: int = 1) -> int:
        """Up to `iterations` more iterations of every member; the number of members still running."""
        a = ctypes.c_int()
        nat.call("sbmp_kgmt_batch_step", self._h, iterations, ctypes.byref(a))
        return a.value

    def enqueue(self, iterations: int) -> None:
        nat.call("sbmp_kgmt_batch_enqueue", self._h, iterations)

    def sync(self) -> None:
        nat.call("sbmp_kgmt_batch_sync", self._h)

    def result(self, i: int) -> nat.PlanResult:
        r = nat.PlanResult()
        nat.call("sbmp_kgmt_batch_result", self._h, int(i), ctypes.byref(r))
        self._members[i]._absorb(r)
        return r

    def info(self) -> dict:
        """count, groupsPerMember, residentGroups, membersPerLaunch, launchesPerIteration, batched
        (sbmp_batch_info: the packing chosen at the last begin)."""
        b = nat.BatchInfo()
        nat.call("sbmp_kgmt_batch_info", self._h, ctypes.byref(b))
        return {k: getattr(b, k) for k, _ in nat.BatchInfo._fields_}

    def kernel_stats(self) -> dict:
        """{"k_step_batch": (launches, total ms)} with profileKernels; the members' own launches
        are in batch[i].kernel_stats()."""
        s = nat.KernelStat()
        nat.call("sbmp_kgmt_batch_kernel_stat", self._h, ctypes.byref(s))
        return {s.name.decode(): (s.launches, s.totalMs)}

"""Python mirror of the reference planner interface, backed by libsbmp.so.

Reference: class KGMT (include/planners/KGMT.cuh:23-109)
    KGMT(float width, float height, int N, int n, int numIterations, int maxTreeSize,
         int numDisc, float agentLength, float goalThreshold)
    void plan(float* initial, float* goal, float* d_obstacles, int obstaclesCount)
    public fields treeSize_, costToGoal_, numIterations_, maxTreeSize_, numDisc_, width_,
                  height_, agentLength_, goalThreshold_, N_, n_, R1Size_, R2Size_
The reference seeds curand with time(NULL) inside plan() (KGMT.cu:111); here the
seed is an optional keyword (default: time(NULL) converted int -> unsigned long
long exactly as the reference's initCurandStates(..., int seed) call does).
"""
from __future__ import annotations

import ctypes
import time
from typing import Optional

import numpy as np

from . import _native as nat

AGENTS = {"car": nat.SBMP_AGENT_CAR, "point": nat.SBMP_AGENT_POINT}
BATCH_RULES = {"reference": nat.SBMP_BATCH_REFERENCE, "fill": nat.SBMP_BATCH_FILL}


def reference_seed_from_time(t: Optional[float] = None) -> int:
    """time(NULL) -> int -> unsigned long long (sign-extended), as KGMT.cu:111 + curand_init."""
    v = ctypes.c_int(int(time.time() if t is None else t)).value
    return v & 0xFFFFFFFFFFFFFFFF


class DeviceBuffer:
    """A float32 device array allocated through the ABI (demos/main.cu:60-61 cudaMalloc+cudaMemcpy)."""

    def __init__(self, host: np.ndarray):
        host = np.ascontiguousarray(host, dtype=np.float32).ravel()
        p = ctypes.c_void_p()
        nat.call("sbmp_device_upload_f32", host.ctypes.data_as(ctypes.c_void_p), host.size, ctypes.byref(p))
        self.ptr = p.value or 0
        self.count = host.size

    def free(self):
        if self.ptr:
            nat.call("sbmp_device_free", ctypes.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_ptr(obj) -> int:
    """Device address of a DeviceBuffer, a torch tensor on the GPU, or a raw int."""
    if obj is None:
        return 0
    if isinstance(obj, DeviceBuffer):
        return obj.ptr
    if isinstance(obj, int):
        return obj
    if hasattr(obj, "data_ptr"):
        if hasattr(obj, "is_cuda") and not obj.is_cuda:
            raise ValueError("d_obstacles must live in device memory")
        return obj.data_ptr()
    raise TypeError(f"cannot take a device pointer of {type(obj)!r}")


def random_tree(kind: str, root, rows: int = 0, blocks: int = 0, threads_per_block: int = 0, device: int = 0):
    """Legacy random-tree generators of the reference's Planner interface:
    kind 'naive' (NaivePlanner.cu) or 'costprop' (CostPropPlanner.cu); sizes <= 0 take the
    reference's.  Returns (samples (rows, blocks * threads_per_block, 7) float32, kernel ms)."""
    naive = kind == "naive"
    if kind not in ("naive", "costprop"):
        raise ValueError("kind must be 'naive' or 'costprop'")
    rows = rows if rows > 0 else (10 if naive else 1)
    blocks = blocks if blocks > 0 else (32 if naive else 512)
    tpb = threads_per_block if threads_per_block > 0 else (32 if naive else 1024)
    r = np.zeros(7, dtype=np.float32)
    r[: len(root)] = np.asarray(root, dtype=np.float32)[:7]
    out = np.zeros((rows, blocks * tpb, 7), dtype=np.float32)
    ms = ctypes.c_float()
    nat.call("sbmp_random_tree", device, 0 if naive else 1, r.ctypes.data_as(ctypes.c_void_p), rows, blocks, tpb,
             out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(ms))
    return out, ms.value


def read_obstacles_csv(path: str, workspace_dim: int = 2) -> np.ndarray:
    """readObstaclesFromCSV (reference src/helper/helper.cu:11-34) through the ABI; (count, 4) float32."""
    n = ctypes.c_int()
    nat.call("sbmp_read_obstacles_csv", path.encode(), workspace_dim, None, 0, ctypes.byref(n))
    cap = max(1, n.value * 2 * workspace_dim + 2 * workspace_dim)
    buf = np.zeros(cap, dtype=np.float32)
    nat.call("sbmp_read_obstacles_csv", path.encode(), workspace_dim, buf.ctypes.data_as(ctypes.c_void_p), cap,
             ctypes.byref(n))
    return buf[: n.value * 2 * workspace_dim].reshape(n.value, 2 * workspace_dim).copy()


def division_reciprocal(b: float) -> float:
    """RN(1/b) if the kernels divide by b through the verified reciprocal, 0.0 if they take the IEEE
    division (sbmp_division_reciprocal; host-only)."""
    y = ctypes.c_float()
    nat.call("sbmp_division_reciprocal", ctypes.c_float(b), ctypes.byref(y))
    return y.value


def device_count() -> int:
    n = ctypes.c_int()
    nat.call("sbmp_device_count", ctypes.byref(n))
    return n.value


def hbm_copy_bandwidth(nbytes: int = 4 << 30, reps: int = 5) -> float:
    """Measured HBM copy bandwidth of the current device in GB/s (sbmp_hbm_copy_bandwidth)."""
    g = ctypes.c_double()
    nat.call("sbmp_hbm_copy_bandwidth", ctypes.c_size_t(nbytes), reps, ctypes.byref(g))
    return g.value


def _vec7(v) -> np.ndarray:
    a = np.zeros(7, dtype=np.float32)
    v = np.asarray(v, dtype=np.float32).ravel()
    a[: len(v)] = v
    return a


def _kgmt_params(width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength, goalThreshold,
                samplesPerIteration, agent, fixGNewClear, device, profileKernels, batchRule) -> nat.KgmtParams:
    """sbmp_kgmt_params of KGMT's (and KGMTBatch's) constructor arguments."""
    p = nat.KgmtParams()
    nat.call("sbmp_kgmt_default_params", ctypes.byref(p))
    p.width, p.height, p.N, p.n = width, height, N, n
    p.numIterations, p.maxTreeSize, p.numDisc = numIterations, maxTreeSize, numDisc
    p.agentLength, p.goalThreshold = agentLength, goalThreshold
    p.samplesPerIteration = samplesPerIteration
    p.agent = AGENTS[agent]
    p.fixGNewClear = int(bool(fixGNewClear))
    p.device = device
    p.profileKernels = int(bool(profileKernels))
    p.batchRule = BATCH_RULES[batchRule]
    return p


class KGMT:
    """MI355X KGMT planner with the reference's constructor and plan() signature."""

    def __init__(self, width: float, height: float, N: int, n: int, numIterations: int, maxTreeSize: int,
                 numDisc: int, agentLength: float, goalThreshold: float, *, samplesPerIteration: int = 0,
                 agent: str = "car", fixGNewClear: bool = False, device: int = 0, profileKernels: bool = False,
                 batchRule: str = "reference", _sharded=None, _local_group: int = 0, _host_sharded=None):
        p = _kgmt_params(width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength, goalThreshold,
                        samplesPerIteration, agent, fixGNewClear, device, profileKernels, batchRule)
        self._params = p
        h = ctypes.c_void_p()
        self._coll = None
        if _local_group:   # sharded data flow with virtual ranks on one device (tests)
            nat.call("sbmp_kgmt_create_local_group", ctypes.byref(p), int(_local_group), ctypes.byref(h))
        elif _host_sharded is not None:   # sharded, collectives by host callbacks (cudasbmp_amd.host_comm)
            coll, nranks, rank = _host_sharded
            self._coll = coll   # the callbacks must outlive the planner
            nat.call("sbmp_kgmt_create_sharded_host", ctypes.byref(p), ctypes.byref(coll.struct), nranks, rank,
                     ctypes.byref(h))
        elif _sharded is None:
            nat.call("sbmp_kgmt_create", ctypes.byref(p), ctypes.byref(h))
        else:
            uid, nranks, rank = _sharded
            idbuf = (ctypes.c_uint8 * nat.SBMP_COMM_ID_BYTES).from_buffer_copy(bytes(uid))
            nat.call("sbmp_kgmt_create_sharded", ctypes.byref(p), idbuf, nranks, rank, ctypes.byref(h))
        self._h = h
        self._set_reference_fields(width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength,
                                   goalThreshold)

    def _set_reference_fields(self, width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength,
                              goalThreshold):
        """The reference's public fields (KGMT.cuh:34-43, 103-106)."""
        self.width_, self.height_, self.N_, self.n_ = float(width), float(height), N, n
        self.numIterations_, self.maxTreeSize_, self.numDisc_ = numIterations, maxTreeSize, numDisc
        self.agentLength_, self.goalThreshold_ = float(agentLength), float(goalThreshold)
        self.R1Size_ = float(np.float32(width) / np.float32(N))
        self.R2Size_ = float(np.float32(width) / np.float32(n * N))
        self.treeSize_ = 0
        self.costToGoal_ = 0.0
        self.last_result: Optional[nat.PlanResult] = None
        self._obs_keepalive = None

    @classmethod
    def from_params(cls, **kw) -> "KGMT":
        base = dict(width=20.0, height=20.0, N=16, n=8, numIterations=100, maxTreeSize=30000, numDisc=10,
                    agentLength=1.0, goalThreshold=0.5)
        base.update(kw)
        return cls(**base)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            nat.call("sbmp_kgmt_destroy", self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def M(self) -> int:
        return self.maxTreeSize_

    # ---------------------------------------------------------------- planning
    def plan(self, initial, goal, d_obstacles, obstaclesCount: int, seed: Optional[int] = None) -> nat.PlanResult:
        """KGMT::plan (reference KGMT.cu:80-317); blocking."""
        seed = reference_seed_from_time() if seed is None else seed
        i, g = _vec7(initial), _vec7(goal)
        r = nat.PlanResult()
        self._obs_keepalive = d_obstacles
        nat.call("sbmp_kgmt_plan", self._h, i.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p),
                 ctypes.c_void_p(device_ptr(d_obstacles)), obstaclesCount, seed, ctypes.byref(r))
        self._absorb(r)
        return r

    def begin(self, initial, goal, d_obstacles, obstaclesCount: int, seed: int) -> None:
        i, g = _vec7(initial), _vec7(goal)
        self._obs_keepalive = d_obstacles
        nat.call("sbmp_kgmt_begin", self._h, i.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p),
                 ctypes.c_void_p(device_ptr(d_obstacles)), obstaclesCount, seed)

    def step(self, iterations: int = 1) -> bool:
        """Run up to `iterations` more loop iterations; False once the loop has ended."""
        a = ctypes.c_int()
        nat.call("sbmp_kgmt_step", self._h, iterations, ctypes.byref(a))
        return bool(a.value)

    def enqueue(self, iterations: int) -> None:
        nat.call("sbmp_kgmt_enqueue", self._h, iterations)

    def sync(self) -> None:
        nat.call("sbmp_kgmt_sync", self._h)

    def fold(self) -> None:
        """Enqueue the R2Valid / R2Invalid fold of every iteration enqueued so far (no wait)."""
        nat.call("sbmp_kgmt_fold", self._h)

    def result(self) -> nat.PlanResult:
        r = nat.PlanResult()
        nat.call("sbmp_kgmt_result", self._h, ctypes.byref(r))
        self._absorb(r)
        return r

    def _absorb(self, r: nat.PlanResult) -> None:
        self.treeSize_ = r.treeSize
        self.costToGoal_ = r.costToGoal
        self.last_result = r

    def stream(self) -> int:
        s = ctypes.c_void_p()
        nat.call("sbmp_kgmt_stream", self._h, ctypes.byref(s))
        return s.value or 0

    # ---------------------------------------------------------------- state export
    def tree(self):
        M = self.M
        s = np.zeros((M, 7), dtype=np.float32)
        p = np.zeros(M, dtype=np.int32)
        c = np.zeros(M, dtype=np.float32)
        nat.call("sbmp_kgmt_copy_tree", self._h, s.ctypes.data_as(ctypes.c_void_p),
                 p.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), M)
        return s, p, c

    def solution_path(self, node: int = -1):
        """Rows root .. node (default: the solution node) with their samples (n, 7) and
        costs; empty arrays when there is no solution."""
        n = ctypes.c_int()
        nat.call("sbmp_kgmt_solution_path", self._h, int(node), None, None, None, 0, ctypes.byref(n))
        rows = np.zeros(n.value, dtype=np.int32)
        s = np.zeros((n.value, 7), dtype=np.float32)
        c = np.zeros(n.value, dtype=np.float32)
        if n.value:
            nat.call("sbmp_kgmt_solution_path", self._h, int(node), rows.ctypes.data_as(ctypes.c_void_p),
                     s.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n))
        return rows, s, c

    def solution_paths(self, nodes) -> dict:
        """The paths root .. node of many nodes in one device pass (sbmp_kgmt_solution_paths;
        include/sbmp/tree_paths.h): nodes is (Q,) rows of tree(), -1 for none (a bestRow of
        query_goals feeds straight in).  Returns lengths (Q,), status (Q,) of SBMP_PATH_* (0 ok,
        1 none, 2 broken, 3 deep), offsets (Q + 1, int64), and the concatenated rows, samples
        (total, 7) and costs in solution_path's layout; path i is [offsets[i], offsets[i + 1])."""
        from .tree_paths import paths_dict
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        n = nodes.ctypes.data_as(ctypes.c_void_p) if len(nodes) else None
        return paths_dict(lambda *o: nat.call("sbmp_kgmt_solution_paths", self._h, n, len(nodes), *o), nodes)

    def trace(self, rows=None):
        """The numDisc Euler states of the edge that ends on each row of `rows` (None: every row
        of the tree), bit for bit what the planner integrated (sbmp_kgmt_trace_rows).  Returns
        (steps (count, numDisc, 4) of (x, y, theta, v), a transposed view of the step-major
        array, status (count,) uint8: SBMP_ROW_FREE, ORPHAN or STALE)."""
        if rows is None:
            n = max(1, min(self.result().treeSize, self.M))
            ptr = None
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            n = len(rows)
            ptr = rows.ctypes.data_as(ctypes.c_void_p) if n else None
        D = self.numDisc_
        steps = np.zeros((D, max(1, n), 4), dtype=np.float32)
        status = np.zeros(max(1, n), dtype=np.uint8)
        nat.call("sbmp_kgmt_trace_rows", self._h, ptr, n, steps.ctypes.data_as(ctypes.c_void_p),
                 status.ctypes.data_as(ctypes.c_void_p))
        return steps[:, :n].transpose(1, 0, 2), status[:n]

    def trajectories(self, nodes) -> dict:
        """solution_paths(nodes) plus `steps` (total, numDisc, 4) and `step_status` (total,): the
        trace of the concatenated path rows, so path i moves through steps[offsets[i] + 1 :
        offsets[i + 1]] (the first row of a path is the root, which has no edge)."""
        out = self.solution_paths(nodes)
        out["steps"], out["step_status"] = self.trace(out["rows"])
        return out

    def resample(self, nodes, period) -> dict:
        """The paths root .. node of many nodes as set-points on one clock, one every `period`
        seconds of path time from the root, in one device pass (sbmp_kgmt_resample_paths;
        include/sbmp/tree_resample.h).  Every set-point lies on the Euler segment the planner
        collision-checked; the last sample of a path is the node as stored, at the path's total
        time.  Returns counts (Q,), status (Q,) of SBMP_PATH_*, offsets (Q + 1, int64), states
        (total, 4) of (x, y, theta, v), edges (total,) (the row whose edge a sample lies on) and
        times (total,) float64; path i is [offsets[i], offsets[i + 1])."""
        from .tree_resample import resample_dict
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        n = nodes.ctypes.data_as(ctypes.c_void_p) if len(nodes) else None
        return resample_dict(lambda *o: nat.call("sbmp_kgmt_resample_paths", self._h, n, len(nodes),
                                                 ctypes.c_double(float(period)), *o), nodes)

    def extract(self, root: int = 0, alive: bool = False) -> dict:
        """The subtree below row `root` as a tree of its own, in one device pass
        (sbmp_kgmt_extract_tree; include/sbmp/tree_extract.h): the rows whose parent chain reaches
        `root` through kept rows only, numbered densely in their old order with their parents
        rewritten.  alive=True keeps the rows the last recheck() left alive; otherwise every row.
        Returns state (kept, 4), ctrl (kept, 4) with the stored cost in column 3, parent (kept,)
        with -1 for the new root, origin (kept,) (the row of tree() a new row came from), newRow
        (rows,) (-1 for a row that is no member) and summary, a dict rows, kept, below, masked,
        detached, root, rootCost.  The plan goes on unchanged."""
        from .tree_extract import extract_dict
        return extract_dict(lambda *o: nat.call("sbmp_kgmt_extract_tree", self._h, int(root), int(bool(alive)), *o), None)

    def adopt(self, samples, parents, costs, goal, d_obstacles, count: int, seed: int, frontier_from: int = 0,
              depth_bound: int = 0) -> dict:
        """Adopt a tree in place of begin() and iteration 1 (sbmp_kgmt_adopt_tree;
        include/sbmp/tree_adopt.h): samples (R, 7), parents (R,), costs (R,) as tree() returns them,
        or state (R, 4), parents, ctrl (R, 4) as extract() does.  Every row is seeded as the root is;
        the loop goes on over the frontier, the rows [frontier_from, R).  depth_bound: the rows of
        the longest parent chain (0: R).  Returns the summary, a dict rows, nonFinite,
        frontierNonFinite, outOfGrid, goalRow, treeSize, gLo; step(), result(), tree(), regions(),
        iter_log() and every tree pass then work as after begin(), row 1 of iter_log() being the
        adoption."""
        from .tree_adopt import adopt
        return adopt(self, samples, parents, costs, goal, d_obstacles, count, seed, frontier_from, depth_bound)

    def replan(self, goal, d_obstacles, count: int, seed: int, root: int = 0, alive: bool = False,
               frontier_from: int = 0) -> dict:
        """extract(root, alive) of the planner's own tree, on the device, adopted against another
        goal and obstacle list (sbmp_kgmt_replan); frontier_from counts in the extracted numbering."""
        from .tree_adopt import replan
        return replan(self, goal, d_obstacles, count, seed, root, alive, frontier_from)

    def reanchor(self, state, root: int = 0, obstacles=(), obstaclesCount: Optional[int] = None) -> dict:
        """The subtree below row `root` re-anchored on the measured state (x, y, theta, v)
        (sbmp_kgmt_reanchor_tree; include/sbmp/tree_reanchor.h): extract(root) with every row kept,
        then every row replayed from its parent's new state with its stored controls against
        `obstacles` ((n, 4) array, or a device pointer with obstaclesCount), one launch per level.
        Returns, in the extracted numbering, state (rows, 4) with the new states (a dead row keeps
        its stored one), ctrl, parent, origin, status (SBMP_ROW_*), alive (rows,) uint8 and summary,
        a dict rows, alive, blocked, orphan, cut, firstDead, levels.  The plan goes on unchanged."""
        from .tree_reanchor import reanchor
        return reanchor(self, state, root, obstacles, obstaclesCount)

    def replan_from(self, state, goal, d_obstacles, count: int, seed: int, root: int = 0,
                    frontier_from: int = 0) -> dict:
        """reanchor(state, root) against d_obstacles, the rows that stay alive extracted, and the
        result adopted against `goal` and d_obstacles, all on the device (sbmp_kgmt_replan_from);
        frontier_from counts in the final numbering.  Returns {"reanchor": summary, "adopt": summary}."""
        from .tree_reanchor import replan_from
        return replan_from(self, state, goal, d_obstacles, count, seed, root, frontier_from)

    def query_goals(self, goals, radius=None, alive: bool = False) -> dict:
        """Goal discs against the tree as it stands (sbmp_kgmt_query_goals; one k_tree_query pass
        per 16 goals): goals is (Q, 2) with one radius for all, or (Q, 3) rows of (x, y, radius).
        Returns (Q,) arrays count, firstRow, bestRow, bestCost, nearestRow, nearestDistance over
        the rows tree() exports; the plan goes on unchanged.  alive=True: over the rows the last
        recheck() left alive only (sbmp_kgmt_query_goals_alive); row numbers stay the tree's own."""
        from .tree_query import ANSWER_DTYPE, answers_dict, goal_array
        g = goal_array(goals, radius)
        out = np.zeros(max(1, len(g)), dtype=ANSWER_DTYPE)
        nat.call("sbmp_kgmt_query_goals_alive" if alive else "sbmp_kgmt_query_goals", self._h,
                 g.ctypes.data_as(ctypes.c_void_p), len(g), out.ctypes.data_as(ctypes.c_void_p))
        return answers_dict(out[: len(g)])

    def recheck(self, obstacles, obstaclesCount: Optional[int] = None):
        """The tree as it stands re-checked against another obstacle list (sbmp_kgmt_recheck_tree;
        include/sbmp/tree_recheck.h): obstacles is an (n, 4) array, or a device pointer with
        obstaclesCount as plan() takes them.  Returns (status, summary): one byte per row of
        tree() up to min(treeSize, M) (SBMP_ROW_*; bit 7, SBMP_ROW_CUT, on a free row below a dead
        one) and a dict rows, alive, blocked, stale, orphan, cut, firstDead.  The plan, its own
        obstacle list and what it goes on to compute are unchanged."""
        s = nat.TreeRecheck()
        own = None
        try:
            if obstaclesCount is None:
                boxes = np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 4)
                obstaclesCount = len(boxes)
                own = DeviceBuffer(boxes) if obstaclesCount else None
                ptr = own.ptr if own is not None else None
            else:
                ptr = device_ptr(obstacles) if obstaclesCount else None
            status = np.zeros(max(1, self.M), dtype=np.uint8)
            nat.call("sbmp_kgmt_recheck_tree", self._h, ctypes.c_void_p(ptr), int(obstaclesCount),
                     status.ctypes.data_as(ctypes.c_void_p), len(status), ctypes.byref(s))
        finally:
            if own is not None:
                own.free()
        return status[: s.rows].copy(), {k: getattr(s, k) for k, _ in nat.TreeRecheck._fields_}

    def unexplored(self):
        M = self.M
        s = np.zeros((M, 7), dtype=np.float32)
        p = np.zeros(M, dtype=np.int32)
        nat.call("sbmp_kgmt_copy_unexplored", self._h, s.ctypes.data_as(ctypes.c_void_p),
                 p.ctypes.data_as(ctypes.c_void_p), M)
        return s, p

    def flags(self):
        M = self.M
        g = np.zeros(M, dtype=np.uint8)
        gn = np.zeros(M, dtype=np.uint8)
        nat.call("sbmp_kgmt_copy_flags", self._h, g.ctypes.data_as(ctypes.c_void_p),
                 gn.ctypes.data_as(ctypes.c_void_p), M)
        return g, gn

    def regions(self) -> dict:
        n1 = self.N_ * self.N_
        n2 = n1 * self.n_ * self.n_
        r = {k: np.zeros(n1, dtype=np.int32) for k in ("R1", "R1Avail", "R1Valid", "R1Invalid")}
        r["R1Score"] = np.zeros(n1, dtype=np.float32)
        for k in ("R2Avail", "R2Valid", "R2Invalid"):
            r[k] = np.zeros(n2, dtype=np.int32)
        order = ("R1", "R1Avail", "R1Valid", "R1Invalid", "R1Score", "R2Avail", "R2Valid", "R2Invalid")
        nat.call("sbmp_kgmt_copy_regions", self._h, *[r[k].ctypes.data_as(ctypes.c_void_p) for k in order])
        return r

    def num_slots(self) -> int:
        n = ctypes.c_int()
        nat.call("sbmp_kgmt_num_slots", self._h, ctypes.byref(n))
        return n.value

    def rng(self) -> np.ndarray:
        n = self.num_slots()
        out = np.zeros((n, 6), dtype=np.uint32)
        nat.call("sbmp_kgmt_copy_rng", self._h, out.ctypes.data_as(ctypes.c_void_p), n)
        return out

    def iter_log(self) -> np.ndarray:
        cnt = ctypes.c_int()
        nat.call("sbmp_kgmt_iter_log", self._h, None, 0, ctypes.byref(cnt))
        arr = (nat.IterRecord * max(1, cnt.value))()
        nat.call("sbmp_kgmt_iter_log", self._h, ctypes.cast(arr, ctypes.c_void_p), cnt.value, ctypes.byref(cnt))
        return np.array([[getattr(arr[i], k) for k in nat.ITER_FIELDS] for i in range(cnt.value)],
                        dtype=np.int64).reshape(-1, len(nat.ITER_FIELDS))

    def export_csv(self, directory: str) -> None:
        """The 13 CSV dumps of KGMT.cu:299-311."""
        nat.call("sbmp_kgmt_export_csv", self._h, directory.encode())

    def set_iteration_dump(self, directory: Optional[str]) -> None:
        """Per-iteration Data/<Kind>/<kind><itr>.csv dumps during plan() (KGMT.cu:263-290); None: off."""
        nat.call("sbmp_kgmt_set_iteration_dump", self._h, directory.encode() if directory else None)

    def kernel_stats(self) -> dict:
        cnt = ctypes.c_int()
        arr = (nat.KernelStat * 16)()
        nat.call("sbmp_kgmt_kernel_stats", self._h, ctypes.cast(arr, ctypes.c_void_p), 16, ctypes.byref(cnt))
        return {arr[i].name.decode(): (arr[i].launches, arr[i].totalMs) for i in range(min(cnt.value, 16))}

    def reset_kernel_stats(self) -> None:
        nat.call("sbmp_kgmt_reset_kernel_stats", self._h)

    OBSTACLE_FORMS = ("registers", "lds", "grid", "global")
    EXCHANGES = ("none", "oneshot", "collective")
    RCP_DIVISORS = (("R1Size", 1), ("R2Size", 2), ("numDisc", 4), ("agentLength", 8))   # SBMP_RCP_*

    def path_info(self) -> dict:
        """The form of the hot path chosen at the last begin() (sbmp_kgmt_path_info)."""
        pi = nat.PathInfo()
        nat.call("sbmp_kgmt_path_info", self._h, ctypes.byref(pi))
        return {"form": "k_step" if pi.stepForm else "two-launch",
                "obstacle_form": self.OBSTACLE_FORMS[pi.obstacleForm] if 0 <= pi.obstacleForm < 4 else pi.obstacleForm,
                "resident_groups": pi.residentGroups, "needed_groups": pi.neededGroups,
                "exchange": self.EXCHANGES[pi.exchange] if 0 <= pi.exchange < 3 else pi.exchange,
                "nranks": pi.nranks, "rank": pi.rank, "rccl_nranks": pi.commRanks,
                "list_mirror": bool(pi.listMirror), "fused_exchange": bool(pi.fusedExchange),
                "oneshot_check": {0: "not run", 1: "passed", -1: "failed"}.get(pi.oneshotCheck, pi.oneshotCheck),
                "mirror_check": {0: "not run", 1: "passed", -1: "failed"}.get(pi.mirrorCheck, pi.mirrorCheck),
                "fused_check": {0: "not run", 1: "passed", -1: "failed"}.get(pi.fusedCheck, pi.fusedCheck),
                "row_table_lds": bool(pi.rowTableLds),
                "rcp_divisions": {k: bool(pi.rcpDivisions & b) for k, b in self.RCP_DIVISORS}}

    def kernel_samples(self, name: str) -> np.ndarray:
        """Per-launch durations (ms) of kernel `name` since the last reset_kernel_stats()."""
        cnt = ctypes.c_int()
        nat.call("sbmp_kgmt_kernel_samples", self._h, name.encode(), None, 0, ctypes.byref(cnt))
        out = np.zeros(max(1, cnt.value), dtype=np.float32)
        nat.call("sbmp_kgmt_kernel_samples", self._h, name.encode(), out.ctypes.data_as(ctypes.c_void_p),
                 cnt.value, ctypes.byref(cnt))
        return out[: cnt.value]

    def enqueue_delay(self, microseconds: float) -> None:
        """Hold the stream for a bounded time so the launches queued next run back to back."""
        nat.call("sbmp_kgmt_enqueue_delay", self._h, float(microseconds))

    def set_profiling(self, enabled: bool) -> None:
        nat.call("sbmp_kgmt_set_profiling", self._h, int(bool(enabled)))

    def state_hash(self) -> int:
        """64-bit digest of the replicated state (tree, tables, control blocks): equal on every rank."""
        h = ctypes.c_uint64()
        nat.call("sbmp_kgmt_state_hash", self._h, ctypes.byref(h))
        return int(h.value)


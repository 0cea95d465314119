/* sbmp.h — C ABI of the MI355X-native KGMT planner (libsbmp.so).
 *
 * The reference (nipe1783/cudaSBMP) exposes one planner, the C++ class KGMT
 * (reference include/planners/KGMT.cuh:23-109), driven by demos/main.cu.  This
 * ABI is the thin, plain-pointer boundary that replaces it; the C++ facade in
 * include/planners/KGMT.h rebuilds the reference's class on top of it, so
 * demos/main.cpp stays a drop-in for demos/main.cu.
 *
 * Conventions
 *   - Every call returns sbmp_status (0 = SBMP_OK).  On failure
 *     sbmp_last_error() describes the cause.  (The reference has no error
 *     codes: CUDA_ERROR_CHECK prints and exit(1)s, include/helper/helper.cuh:19-27,
 *     and the KGMT kernel launches are unchecked.)
 *   - Host arrays are plain C arrays; device arrays are HIP device pointers
 *     (d_ prefix), exactly as the reference's plan() takes d_obstacles.
 *   - One planner handle = one HIP stream on one device; a handle is not
 *     thread-safe.  plan()/begin() may be called repeatedly on one handle
 *     (the reference's plan() is single-shot: it frees ctor-owned buffers,
 *     KGMT.cu:314-316).
 */
#ifndef SBMP_H
#define SBMP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBMP_ABI_VERSION 1

typedef int sbmp_status;
#define SBMP_OK 0
#define SBMP_ERR_INVALID_ARGUMENT 1
#define SBMP_ERR_HIP 2
#define SBMP_ERR_IO 3
#define SBMP_ERR_OUT_OF_MEMORY 4
#define SBMP_ERR_STATE 5
#define SBMP_ERR_UNSUPPORTED 6
#define SBMP_ERR_COMM 7

#define SBMP_AGENT_CAR 0   /* kinematic bicycle, reference src/statePropagator/statePropagator.cu:5-76 */
#define SBMP_AGENT_POINT 1 /* holonomic R2 point (build extension, no reference counterpart) */

#define SBMP_SAMPLE_DIM 7  /* [x, y, theta, v, a, steering, duration], reference KGMT.cu:5, State.h:6-20 */

/* Constructor arguments of KGMT::KGMT (reference KGMT.cuh:28, KGMT.cu:10-78)
 * plus the build's knobs. */
typedef struct sbmp_kgmt_params {
    float width, height;      /* workspace extent */
    int N, n;                 /* R1 grid N x N (N must be 16, KGMT.cu:8); R2 sub-grid n x n per R1 cell (1..16) */
    int numIterations;        /* loop bound, KGMT.cu:118 */
    int maxTreeSize;          /* tree capacity M */
    int numDisc;              /* Euler sub-steps per child, statePropagator.cu:33 */
    float agentLength;        /* bicycle wheelbase, statePropagator.cu:58 */
    float goalThreshold;      /* goal radius, KGMT.cu:635-638 (0 disables the goal) */
    int samplesPerIteration;  /* 0 = reference batch rule (KGMT.cu:151-219); S > 0 = capped extension */
    int agent;                /* SBMP_AGENT_* */
    int fixGNewClear;         /* 0 = reproduce the reference's partial GNew clear */
    int device;               /* HIP device ordinal */
    int profileKernels;       /* 1 = time every kernel launch with HIP events (sbmp_kgmt_kernel_stats) */
    int batchRule;            /* SBMP_BATCH_REFERENCE or SBMP_BATCH_FILL (needs samplesPerIteration > 0) */
} sbmp_kgmt_params;

/* Children per frontier node.  REFERENCE: 32, or floor(remaining/|G|) once 32|G|
 * exceeds the remaining capacity (KGMT.cu:151-158), with remaining additionally
 * capped at samplesPerIteration when that is > 0.  FILL (build extension D14):
 * floor(samplesPerIteration/|G|) children per frontier node, so every iteration
 * generates (almost exactly) samplesPerIteration children. */
#define SBMP_BATCH_REFERENCE 0
#define SBMP_BATCH_FILL 1

/* Outcome of a plan (the reference's public fields treeSize_/costToGoal_, KGMT.cuh:37,40,
 * plus what its prints report, KGMT.cu:295-296). */
typedef struct sbmp_plan_result {
    int iterations;           /* loop iterations executed */
    int treeSize;             /* treeSize_ (may exceed maxTreeSize on the final iteration, as in the reference) */
    float costToGoal;         /* costToGoal_: cost of the first goal node, 0 if none */
    int goalIndex;            /* tree row of that node, -1 if none (D4: lowest row of the first goal iteration) */
    long long samplesGenerated; /* children propagated and collision-checked, all iterations */
    long long accepted;       /* nodes appended to the tree, all iterations */
    double wallMs;            /* device-synchronised wall time of the iteration loop */
    int stalled;              /* 1 if the loop ended with an empty frontier (D7) */
} sbmp_plan_result;

/* Per-iteration bookkeeping (same fields as the oracle's log). */
typedef struct sbmp_iter_record {
    int itr, treeSizeBefore, nG, k, nExp, S, A, treeSizeAfter, goalIdx;
} sbmp_iter_record;

typedef struct sbmp_kernel_stat {
    char name[32];
    long long launches;
    double totalMs;           /* sum of HIP-event durations on the planner's stream */
} sbmp_kernel_stat;

/* Which form of the hot path a planner runs (sbmp_kgmt_path_info): no reference
 * counterpart (the reference has one form, KGMT.cu:118-292); for logs and bench lines. */
#define SBMP_OBS_REGISTERS 0  /* <= 8 boxes held in registers (wave cull + per-step schedule) */
#define SBMP_OBS_LDS 1        /* <= 2,048 boxes staged in LDS per workgroup */
#define SBMP_OBS_GRID 2       /* uniform-grid obstacle index (include/sbmp/obstacle_grid.h) */
#define SBMP_OBS_GLOBAL 3     /* the all-boxes loop from global memory (diagnostics) */
#define SBMP_EXCHANGE_NONE 0      /* one rank */
#define SBMP_EXCHANGE_ONESHOT 1   /* k_oneshot through IPC-mapped inboxes (sharded default) */
#define SBMP_EXCHANGE_COLLECTIVE 2 /* the communicator's all-reduce (RCCL, or host callbacks) */
typedef struct sbmp_path_info {
    int stepForm;             /* 1: one k_step launch per iteration; 0: k_expand + k_finish (+ k_pack) */
    int obstacleForm;         /* SBMP_OBS_* of the last begin() */
    int residentGroups;       /* k_step workgroups the device holds at once (occupancy x CUs), 0 if not k_step-capable */
    int neededGroups;         /* 1 + blocks per rank: k_step needs them all resident */
    int exchange;             /* SBMP_EXCHANGE_* */
    int nranks, rank;
    int commRanks;            /* ranks of the RCCL communicator (0: none) */
    int listMirror;           /* 1: the one-shot exchange copies the flagged-children lists into each
                                 rank's mirror, and k_step reads its parents from local HBM */
    int fusedExchange;        /* 1: the last expanding workgroup of k_step runs the one-shot exchange
                                 (no k_oneshot launch) */
    int oneshotCheck;         /* start-up check of the one-shot exchange: 0 not run, 1 passed,
                                 -1 failed on some rank (every rank then uses the all-reduce) */
    int mirrorCheck;          /* start-up check of the list mirror (stores into peers' mirrors
                                 seen after a kernel boundary): 0 not run, 1 passed, -1 failed
                                 on some rank (every rank then reads the lists over the mapping) */
    int fusedCheck;           /* start-up check of the fused exchange's in-kernel order (pushes
                                 drained, relaxed arrivals, the workers' flags, the peers' next
                                 launch reading the mirror): 0 not run, 1 passed, -1 failed on some
                                 rank (every rank then runs the exchange as its own k_oneshot) */
    int rowTableLds;          /* sharded k_step: 1 stages the exchange's u16 block counts in LDS
                                 (row positions without a dependent load); 0 reads a row's block
                                 words (chosen when the table's LDS would cost residency) */
    int rcpDivisions;         /* SBMP_RCP_* bits: the divisors whose divisions the kernels serve with the
                                 host-verified reciprocal (sbmp_division_reciprocal != 0) since the last
                                 begin(); a clear bit is an IEEE division.  The binning of a child
                                 (bins_k) takes the reciprocal only with both R1Size and R2Size set */
} sbmp_path_info;
#define SBMP_RCP_R1SIZE 1
#define SBMP_RCP_R2SIZE 2
#define SBMP_RCP_NUMDISC 4
#define SBMP_RCP_AGENTLENGTH 8

typedef struct sbmp_kgmt sbmp_kgmt;

int sbmp_abi_version(void);
const char* sbmp_status_string(sbmp_status s);
const char* sbmp_last_error(void);

/* The demo configuration, reference demos/main.cu:19-28. */
sbmp_status sbmp_kgmt_default_params(sbmp_kgmt_params* p);

/* A system / workspace file (systems/NAME.yaml): the reference hardcodes
 * this in demos/main.cu:19-46 and leaves systems/car.yaml empty.  Flat "key: value"
 * lines over the demo defaults: agent, width, height, N, n, numIterations, maxTreeSize,
 * numDisc, agentLength, goalThreshold, samplesPerIteration, batchRule (reference | fill),
 * fixGNewClear, device, initial / goal ([7 values] or a CSV file such as
 * configurations/init/init.csv), obstacles (a CSV path, resolved against the file's
 * directory).  Numeric keys may name a file holding the number.  Unknown keys fail. */
typedef struct sbmp_system_config {
    sbmp_kgmt_params params;
    float initial[7];
    float goal[7];
    char obstacles[1024];     /* resolved path, "" if the file names none */
} sbmp_system_config;
sbmp_status sbmp_load_system_config(const char* path, sbmp_system_config* out);

/* KGMT::KGMT (KGMT.cu:10-78): allocates every planner buffer on p->device. */
sbmp_status sbmp_kgmt_create(const sbmp_kgmt_params* p, sbmp_kgmt** out);
sbmp_status sbmp_kgmt_destroy(sbmp_kgmt* h);

/* KGMT::plan (KGMT.cu:80-317): root init, RNG init (curand_init(seed, slot, 0),
 * KGMT.cu:111 — the reference seeds with time(NULL); here the seed is explicit),
 * iterate until goal / full tree / numIterations.  initial and goal are host
 * arrays of 7 floats; d_obstacles is a device array of obstaclesCount boxes
 * [xmin, ymin, xmax, ymax] (reference collisionCheck.cu:7-14).  Blocking.
 * plan is begin + the loop, so begin's reuse contract (below) holds: any number of plans
 * on one handle, each with its own start, goal, seed and obstacle list. */
sbmp_status sbmp_kgmt_plan(sbmp_kgmt* h, const float initial[7], const float goal[7], const float* d_obstacles,
                           int obstaclesCount, uint64_t seed, sbmp_plan_result* result);

/* Stepwise form of plan: begin = prologue (KGMT.cu:84-116); step enqueues up to
 * `iterations` more loop iterations and waits for them (*active = 0 once the
 * loop has ended); result reads the outcome.
 * Reuse: begin may be called on a handle in any state -- never begun, finished,
 * mid-plan, or with iterations enqueued and not waited for (they are ordered before
 * begin's own work on the handle's stream and their results are dropped).  The plan that
 * follows is the one a fresh handle of the same parameters would compute, bit for bit.
 * The obstacle list may change in length and in form (registers, LDS, grid, none) from
 * call to call.  The caller's array is copied during the call: on return it may be
 * overwritten or freed.  The alive mask of a re-check (sbmp_kgmt_recheck_tree) does not
 * survive begin: sbmp_kgmt_query_goals_alive fails with SBMP_ERR_STATE until the next
 * re-check.  tests/test_gpu_reuse_scenarios.py holds the contract. */
sbmp_status sbmp_kgmt_begin(sbmp_kgmt* h, const float initial[7], const float goal[7], const float* d_obstacles,
                            int obstaclesCount, uint64_t seed);
sbmp_status sbmp_kgmt_step(sbmp_kgmt* h, int iterations, int* active);
/* Enqueue iterations without waiting (device-resident loop; kernels become
 * no-ops once the loop has ended).  sbmp_kgmt_sync waits for the stream. */
sbmp_status sbmp_kgmt_enqueue(sbmp_kgmt* h, int iterations);
sbmp_status sbmp_kgmt_sync(sbmp_kgmt* h);
/* Enqueue, without waiting, the fold of R2Valid / R2Invalid (KGMT.cu:405,410) over
 * every iteration enqueued so far.  The loop folds its per-child key log every 32
 * iterations; exports fold the rest themselves.  A timed window calls this before
 * its closing sync so the deferred work of its own iterations is inside it. */
sbmp_status sbmp_kgmt_fold(sbmp_kgmt* h);
sbmp_status sbmp_kgmt_result(sbmp_kgmt* h, sbmp_plan_result* result);
/* The HIP stream (hipStream_t) every kernel of this planner runs on. */
sbmp_status sbmp_kgmt_stream(sbmp_kgmt* h, void** stream);

/* State export in the reference's layouts (thrust vectors of KGMT.cuh:44-68):
 * samples M x 7 AoS, parents M, costs M, bools as bytes.  capacity = rows of
 * the caller's arrays (must be >= maxTreeSize).  Any pointer may be NULL. */
sbmp_status sbmp_kgmt_copy_tree(sbmp_kgmt* h, float* samples, int* parent, float* costs, int capacity);
sbmp_status sbmp_kgmt_copy_unexplored(sbmp_kgmt* h, float* samples, int* uParent, int capacity);
sbmp_status sbmp_kgmt_copy_flags(sbmp_kgmt* h, uint8_t* G, uint8_t* GNew, int capacity);
/* R1* arrays have N*N entries, R2* arrays N*N*n*n. */
sbmp_status sbmp_kgmt_copy_regions(sbmp_kgmt* h, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid, float* R1Score,
                                   int* R2Avail, int* R2Valid, int* R2Invalid);
/* XORWOW state per slot: 6 words {v0..v4, d}.  Slots = sbmp_kgmt_num_slots. */
sbmp_status sbmp_kgmt_num_slots(sbmp_kgmt* h, int* slots);
sbmp_status sbmp_kgmt_copy_rng(sbmp_kgmt* h, uint32_t* states, int capacity);
sbmp_status sbmp_kgmt_iter_log(sbmp_kgmt* h, sbmp_iter_record* out, int capacity, int* count);
/* The 13 CSV dumps of KGMT.cu:299-311 (std::fixed, 10 decimals, helper.cuh:53-72) into dir. */
sbmp_status sbmp_kgmt_export_csv(sbmp_kgmt* h, const char* dir);
/* The per-iteration dumps the reference has commented out (KGMT.cu:263-290), read by
 * visualization/visualizationKGMT_Steps.m: with dir set, sbmp_kgmt_plan runs one
 * iteration at a time (one host sync each) and after iteration itr writes
 * dir/Data/{Samples/samples, Parents/parents, R1Scores/R1Scores, R1Avail/R1Avail,
 * R1/R1, UnexploredSamples/unexploredSamples}<itr>.csv in the export format.
 * dir NULL or "": off (the default). */
sbmp_status sbmp_kgmt_set_iteration_dump(sbmp_kgmt* h, const char* dir);

/* Solution path (the reference keeps only the goal node's cost,
 * KGMT.cu:586-591): the tree rows from the root to `node` (node < 0: the
 * solution node, result goalIndex), root first, found by walking treeParent.
 * rows (ints), samples (7 floats per row, the samples.csv layout of
 * KGMT.cu:299) and costs may each be NULL; capacity = their length in rows.
 * *length = the path length (0 if node < 0 and there is no solution); with
 * capacity < *length the call fails with SBMP_ERR_INVALID_ARGUMENT (and still sets
 * *length), so a NULL/0 call returns the size to allocate. */
sbmp_status sbmp_kgmt_solution_path(sbmp_kgmt* h, int node, int* rows, float* samples, float* costs, int capacity,
                                    int* length);

/* Goal queries against the tree as it stands (include/sbmp/tree_query.h states the rule;
 * no reference counterpart: the reference asks its tree one question, KGMT.cu:635-638).
 * A row (x, y) is inside goal (x, y, radius) iff sqrtf(dx * dx + dy * dy) < radius, the
 * planner's own goal test (D18): never for radius <= 0 or NaN; radius = +inf takes every row. */
typedef struct sbmp_goal_query {
    float x, y, radius;
} sbmp_goal_query;
typedef struct sbmp_goal_answer {
    int count;                /* rows inside */
    int firstRow;             /* lowest row inside, -1 if none */
    int bestRow;              /* the inside row of lowest cost (lowest row on ties), -1 if none */
    float bestCost;           /* its cost, 0 if none */
    int nearestRow;           /* the row of lowest squared distance over all rows (lowest row on ties) */
    float nearestDistance;    /* sqrtf of that squared distance */
} sbmp_goal_answer;
/* A masked query (sbmp_kgmt_query_goals_alive, sbmp_tree_query_alive_batch) skips a row iff its
 * alive byte is 0 (any non-zero byte is alive) and answers over the rest, row numbers the
 * tree's own.  With no alive row: count 0, firstRow -1, bestRow -1, bestCost 0, nearestRow -1,
 * nearestDistance +inf. */
/* out[i] answers goals[i] over the rows [0, min(treeSize, maxTreeSize)) after everything
 * enqueued has finished: exactly the rows sbmp_kgmt_copy_tree exports, the root included
 * (firstRow equals the plan's goalIndex whenever the root lies outside the disc).  One pass
 * of k_tree_query over the tree per 16 goals, on the planner's stream; it only reads the
 * planner's state, so it may be called after plan() and between step() / enqueue() calls
 * and does not change what the plan goes on to compute.  Also valid on a batch member.
 * Before the first begin(): SBMP_ERR_STATE.  goals or out NULL with count > 0, count < 0,
 * or a goal with a non-finite x or y: SBMP_ERR_INVALID_ARGUMENT.  count == 0 is a no-op. */
sbmp_status sbmp_kgmt_query_goals(sbmp_kgmt* h, const sbmp_goal_query* goals, int count, sbmp_goal_answer* out);

/* Re-check of the tree as it stands against another obstacle list (include/sbmp/tree_recheck.h
 * states the rule; no reference counterpart).  Every row r of [0, rows),
 * rows = min(treeSize, maxTreeSize), gets one status byte, the first matching rule:
 *   SBMP_ROW_FREE     r == 0 (the root has no edge), or the replay of treeState[parent] with
 *                     the row's stored (a, steering, duration) runs all numDisc steps valid
 *                     under the new list and ends on the stored state bit for bit
 *   SBMP_ROW_ORPHAN   r > 0 and parent is not in [0, r) (nothing is read through it)
 *   SBMP_ROW_BLOCKED  the replay meets a box of the new list or leaves the workspace
 *   SBMP_ROW_STALE    the replay stays valid but does not end on the stored state
 * A row is alive iff it is FREE and its parent is alive (row 0: iff FREE, i.e. always).
 * A FREE row that is not alive is exported with SBMP_ROW_CUT set. */
#define SBMP_ROW_FREE 0
#define SBMP_ROW_ORPHAN 1
#define SBMP_ROW_BLOCKED 2
#define SBMP_ROW_STALE 3
#define SBMP_ROW_CUT 0x80
typedef struct sbmp_tree_recheck {
    int rows, alive, blocked, stale, orphan, cut;   /* rows = alive + blocked + stale + orphan + cut */
    int firstDead;                                  /* lowest row not alive, -1 if none */
} sbmp_tree_recheck;
/* d_obstacles: obstaclesCount boxes (xmin, ymin, xmax, ymax) in device memory, as plan()
 * takes them; the planner's own list, obstacle form and grid index are not touched, and the
 * plan goes on unchanged (the call only reads the tree; it waits for everything enqueued, like
 * sbmp_kgmt_state_hash, and runs on the planner's stream).  status: host array of `capacity`
 * bytes or NULL.  out->rows is set in every case, so a NULL / 0 call still re-checks and
 * returns the summary.  The alive mask stays with the planner until the next begin()
 * (sbmp_kgmt_query_goals_alive).  Valid after plan() and between step() calls, on a local
 * shard group (rank 0 answers), a sharded rank (its own replica) and a batch member.
 * Before the first begin(): SBMP_ERR_STATE.  obstaclesCount < 0, a NULL list with
 * obstaclesCount > 0, out NULL, or status given with capacity < rows: SBMP_ERR_INVALID_ARGUMENT. */
sbmp_status sbmp_kgmt_recheck_tree(sbmp_kgmt* h, const float* d_obstacles, int obstaclesCount, uint8_t* status,
                                   int capacity, sbmp_tree_recheck* out);
/* sbmp_kgmt_query_goals with every row that is not alive treated as absent (count, firstRow,
 * bestRow and nearestRow alike; row numbers are the tree's own): the rule at sbmp_goal_answer,
 * over the re-check's mask, whose bytes are 0 and 1 and whose root is alive.  SBMP_ERR_STATE without a
 * re-check since the last begin(), or when min(treeSize, maxTreeSize) no longer equals the
 * re-check's rows (the tree grew: re-check again). */
sbmp_status sbmp_kgmt_query_goals_alive(sbmp_kgmt* h, const sbmp_goal_query* goals, int count,
                                        sbmp_goal_answer* out);

/* Many solution paths and the Euler steps of tree rows in one device pass each
 * (include/sbmp/tree_paths.h states the rule; no reference counterpart).
 * The path of a node is the chain node, parent[node], ... down to row 0 over the rows [0, R),
 * R = min(treeSize, maxTreeSize), reported root first; every request gets one status: */
#define SBMP_PATH_OK 0      /* the chain reaches row 0 within depthBound rows; length = its rows */
#define SBMP_PATH_NONE 1    /* node == -1 (a bestRow of sbmp_kgmt_query_goals with nothing inside); length 0 */
#define SBMP_PATH_BROKEN 2  /* a row r > 0 of the chain has no parent in [0, r); length 0 */
#define SBMP_PATH_DEEP 3    /* more than depthBound rows; length 0 */
/* nodes: count requests (host).  lengths (ints) and status (bytes): count entries each, may be
 * NULL.  The paths lie one behind the other in request order, path i at the exclusive sum of
 * lengths[0 .. i): rows (ints), samples (7 floats per row) and costs in the layout of
 * sbmp_kgmt_solution_path; each may be NULL, capacity = their length in rows.  *total = the
 * sum of the lengths, set in every case: with capacity < *total and any of the three given
 * the call fails with SBMP_ERR_INVALID_ARGUMENT, so a NULL / 0 call returns the size to
 * allocate.  depthBound is numIterations + 2, as for sbmp_kgmt_solution_path.  Stricter than
 * that call: it stops at any negative parent, this one reports SBMP_PATH_BROKEN.  A node
 * < -1 or >= R, nodes NULL with count > 0, count < 0 or total NULL: SBMP_ERR_INVALID_ARGUMENT
 * before anything is launched.  count == 0 is a no-op (*total = 0).  Before the first begin():
 * SBMP_ERR_STATE.  The call waits for everything enqueued, runs k_path_walk on the planner's
 * stream over buffers of its own and only reads the tree: valid after plan() and between
 * step() calls, on a local shard group (rank 0 answers), a sharded rank (its own replica) and
 * a batch member; the plan goes on unchanged. */
sbmp_status sbmp_kgmt_solution_paths(sbmp_kgmt* h, const int* nodes, int count, int* lengths, uint8_t* status,
                                     int* rows, float* samples, float* costs, long long capacity, long long* total);
/* The numDisc Euler states of the edge that ends on each listed row: what the planner
 * integrated and collision-checked, bit for bit.  rows: count row numbers of [0, R) (host), or
 * NULL for the rows [0, count), count <= R.  steps (host): numDisc x count x 4 floats,
 * step-major: step j of entry i is the (x, y, theta, v) at steps + 4 * (j * count + i).
 * status (host, count bytes, may be NULL): SBMP_ROW_FREE (the last step is the stored row bit
 * for bit; row 0, whose steps all hold the root), SBMP_ROW_ORPHAN (no usable parent: every
 * step holds the stored row) or SBMP_ROW_STALE.  A listed row outside [0, R), steps NULL or
 * rows NULL with count > R: SBMP_ERR_INVALID_ARGUMENT.  count == 0 is a no-op; otherwise 0 <
 * count < 2^31.  State, waiting and handles as sbmp_kgmt_solution_paths (k_tree_trace). */
sbmp_status sbmp_kgmt_trace_rows(sbmp_kgmt* h, const int* rows, long long count, float* steps, uint8_t* status);
/* The paths of `count` nodes resampled on one clock in one device pass (include/sbmp/tree_resample.h
 * states the rule): set-points every `period` seconds of path time from the
 * root, each on the Euler segment the planner collision-checked, plus the node itself as the
 * last sample.  nodes, statuses, state, waiting and handles as sbmp_kgmt_solution_paths; a
 * request whose status is not SBMP_PATH_OK gets 0 samples.  counts (ints) and status (bytes):
 * count entries each, may be NULL.  Path i of total time T has floor(T / period) + 2 samples,
 * at the exclusive sum of counts[0 .. i): states (4 floats: x, y, theta, v), edges (the row
 * whose edge the sample lies on; the node for the last sample) and times (doubles, seconds from
 * the root; T for the last sample); each may be NULL, capacity = their length in samples.
 * *total = the sum of the counts, set in every case: with capacity < *total and any of the
 * three given the call fails with SBMP_ERR_INVALID_ARGUMENT, so a NULL / 0 call returns the
 * size to allocate.  period not finite or <= 0, or a path with T / period >= 2^31 - 2:
 * SBMP_ERR_INVALID_ARGUMENT.  Only reads the tree (k_path_walk, k_resample_clock,
 * k_path_resample on the planner's stream over buffers of the call's own). */
sbmp_status sbmp_kgmt_resample_paths(sbmp_kgmt* h, const int* nodes, int count, double period, int* counts,
                                     uint8_t* status, float* states, int* edges, double* times, long long capacity,
                                     long long* total);

/* The usable subtree as a tree of its own: prune and re-root (include/sbmp/tree_extract.h states
 * the rule; no reference counterpart).  Over the rows [0, R), R = min(treeSize,
 * maxTreeSize), a row is a member iff its parent chain reaches `root` through kept rows only;
 * the members are numbered densely in their old order (the root becomes row 0), their parents
 * rewritten, and their stored state and controls copied bit for bit, costs included: costs stay
 * measured from the original root, and rootCost is the stored cost of `root`.  Every row has
 * one class, the first match: below (r < root), masked (not kept), detached (kept, but its
 * parent is no member), kept. */
typedef struct sbmp_tree_extract {
    int rows, kept, below, masked, detached;   /* rows = kept + below + masked + detached */
    int root;
    float rootCost;                            /* ctrl[root].w as stored */
} sbmp_tree_extract;
/* useAlive != 0: a row is kept iff the last sbmp_kgmt_recheck_tree left it alive (SBMP_ERR_STATE
 * without a re-check since the last begin(), or when the tree has grown since, exactly as
 * sbmp_kgmt_query_goals_alive); 0: every row is kept.  Host outputs, each may be NULL: state and
 * ctrl (4 floats per member), parent and origin (the member's old row) hold `capacity` rows,
 * newRow holds R ints (the new row of every old row, -1 for a row that is no member).  *out is
 * set in every case: with capacity < out->kept and any of the four member-sized outputs given the
 * call fails with SBMP_ERR_INVALID_ARGUMENT, so a NULL / 0 call returns the size to allocate.  A
 * root that is not kept gives kept = 0: an answer, not an error.  root outside [0, R) or out
 * NULL: SBMP_ERR_INVALID_ARGUMENT.  Before the first begin(): SBMP_ERR_STATE.  State, waiting
 * and handles as sbmp_kgmt_solution_paths: it only reads the tree (k_extract_* on the planner's
 * stream over buffers of the call's own), and the plan goes on unchanged. */
sbmp_status sbmp_kgmt_extract_tree(sbmp_kgmt* h, int root, int useAlive, float* state, float* ctrl, int* parent,
                                   int* origin, int* newRow, long long capacity, sbmp_tree_extract* out);

/* Adopt a tree into a planner and plan on (include/sbmp/tree_adopt.h states the rule; DESIGN.md
 * §5.14; no reference counterpart).  The adoption takes the place of begin() and of iteration 1:
 * every one of the `rows` rows is seeded as the reference seeds its root (its R1 cell counted
 * in R1 and R1Valid and made available, its R2 bit set, R1Cov the set bits of each R1 cell; a
 * cell of -1 is not counted), the slots are re-seeded from `seed`, and the loop goes on with
 * iteration 2 over the frontier, the row range [frontierFrom, rows): 0 expands every adopted
 * row, `rows` none (the loop then runs without effect, D7).  The lowest adopted row inside the
 * goal radius ends the plan before anything is expanded; rows == maxTreeSize runs no iteration:
 * both are answers, not errors.  depthBound: an upper bound on the rows of any parent chain of
 * the adopted tree (<= 0: rows); the tree passes add the executed iterations to it.  Row 1 of
 * sbmp_kgmt_iter_log is the adoption (S = A = 0).  After the call every entry works as after
 * sbmp_kgmt_begin.  R1Invalid and the R2 counters start at 0 and costs are taken as stored.
 * rows < 1 or > maxTreeSize, frontierFrom outside [0, rows], a non-finite x, y, theta or v in a
 * row of the frontier, a non-finite goal, a NULL array: SBMP_ERR_INVALID_ARGUMENT, with the
 * handle's previous plan left as it was (rows below the frontier are adopted as stored: nothing
 * integrates from them).  A sharded handle, a local shard group, a batch member, and a planner
 * created with numIterations < 1 (the adoption is iteration 1 and plans iteration 2): SBMP_ERR_STATE.
 * sbmp_plan_result.iterations counts the adoption; stalled looks at the iterations the loop ran. */
typedef struct sbmp_tree_adopt_args {
    const float* state;    /* rows x 4: x, y, theta, v */
    const float* ctrl;     /* rows x 4: the edge's controls, the cost in .w */
    const int* parent;     /* rows */
    int rows;
    int frontierFrom;
    int depthBound;
    int onDevice;          /* nonzero: the three arrays are device memory (an sbmp_tree_extract_batch result) */
} sbmp_tree_adopt_args;
typedef struct sbmp_tree_adopt {
    int rows;
    int nonFinite;           /* rows with a non-finite x, y, theta or v */
    int frontierNonFinite;   /* ... of them in [frontierFrom, rows) */
    int outOfGrid;           /* rows with an R1 or R2 cell of -1 */
    int goalRow;             /* the lowest row inside the goal radius, -1 if none */
    int treeSize, gLo;       /* what iteration 2 starts from: rows, frontierFrom */
} sbmp_tree_adopt;
sbmp_status sbmp_kgmt_adopt_tree(sbmp_kgmt* h, const sbmp_tree_adopt_args* args, const float goal[7],
                                 const float* d_obstacles, int obstaclesCount, uint64_t seed, sbmp_tree_adopt* out);
/* sbmp_kgmt_extract_tree of the handle's own tree (root, useAlive as there) into device memory of
 * the call's own, then sbmp_kgmt_adopt_tree of the result: the copy is needed because the
 * adoption clears the tree arrays.  frontierFrom counts in the extracted numbering.  A root that
 * is not kept (nothing to adopt): SBMP_ERR_INVALID_ARGUMENT, the plan left as it was. */
sbmp_status sbmp_kgmt_replan(sbmp_kgmt* h, int root, int useAlive, int frontierFrom, const float goal[7],
                             const float* d_obstacles, int obstaclesCount, uint64_t seed, sbmp_tree_adopt* out);

/* Re-anchor a tree on a measured state (include/sbmp/tree_reanchor.h states the rule; DESIGN.md
 * §5.15; no reference counterpart).  The tree's root is row 0.  Every row is replayed from its
 * parent's NEW state with the row's stored (a, steering, duration), by the expand step's own
 * Euler loop against the given boxes, level by level from the new root state; each row gets one
 * status byte and one output state:
 *   row 0                    SBMP_ROW_FREE, alive, the new root state
 *   parent not in [0, r)     SBMP_ROW_ORPHAN, dead (nothing is read through it)
 *   parent dead              SBMP_ROW_FREE | SBMP_ROW_CUT, dead, not replayed
 *   parent alive             all numDisc steps valid: SBMP_ROW_FREE, alive, the replay's end state;
 *                            else SBMP_ROW_BLOCKED, dead
 * A dead row keeps its stored state bit for bit.  Controls, parents and costs do not change. */
typedef struct sbmp_tree_reanchor {
    int rows, alive, blocked, orphan, cut;   /* rows = alive + blocked + orphan + cut */
    int firstDead;                           /* lowest row not alive, -1 if none */
    int levels;                              /* 1 + the most edges between a row and the top of its chain */
} sbmp_tree_reanchor;
/* sbmp_kgmt_extract_tree of `root` with every row kept, into memory of the call's own, re-anchored
 * on newRoot (x, y, theta, v) with the handle's agent, numDisc, agentLength, workspace and
 * obstacle-form rule against d_obstacles (device, obstaclesCount boxes).  The answer is in the
 * extracted numbering.  Host outputs, each may be NULL: state (the new states), ctrl, parent and
 * origin as sbmp_kgmt_extract_tree gives them and status (one byte a row) hold `capacity` rows.
 * *out is set in every case, out->rows = the extracted rows: with capacity < out->rows and any of
 * the five given the call fails with SBMP_ERR_INVALID_ARGUMENT, so a NULL / 0 call returns the
 * size to allocate.  A non-finite newRoot, root outside [0, R), a bad obstacle list or out NULL:
 * SBMP_ERR_INVALID_ARGUMENT.  State, waiting and handles as sbmp_kgmt_extract_tree: it only reads
 * the tree, and the plan goes on unchanged. */
sbmp_status sbmp_kgmt_reanchor_tree(sbmp_kgmt* h, int root, const float newRoot[4], const float* d_obstacles,
                                    int obstaclesCount, float* state, float* ctrl, int* parent, int* origin,
                                    uint8_t* status, long long capacity, sbmp_tree_reanchor* out);
/* On the device: extract `root` (every row kept), re-anchor on newRoot against d_obstacles,
 * extract the alive rows, and sbmp_kgmt_adopt_tree of the result with goal, d_obstacles and seed.
 * frontierFrom counts in the final numbering, as for sbmp_kgmt_replan.  reanchorOut (may be NULL)
 * gets the re-anchoring's summary, adoptOut the adoption's.  Refusals and out-of-scope handles
 * are sbmp_kgmt_adopt_tree's, plus a non-finite newRoot; a refusal leaves the previous plan as
 * it was. */
sbmp_status sbmp_kgmt_replan_from(sbmp_kgmt* h, int root, const float newRoot[4], int frontierFrom,
                                  const float goal[7], const float* d_obstacles, int obstaclesCount, uint64_t seed,
                                  sbmp_tree_reanchor* reanchorOut, sbmp_tree_adopt* adoptOut);

sbmp_status sbmp_kgmt_kernel_stats(sbmp_kgmt* h, sbmp_kernel_stat* out, int capacity, int* count);
/* The form of the hot path chosen at the last begin() (sbmp_path_info). */
sbmp_status sbmp_kgmt_path_info(sbmp_kgmt* h, sbmp_path_info* out);
sbmp_status sbmp_kgmt_reset_kernel_stats(sbmp_kgmt* h);
/* Turn per-launch HIP-event timing on/off for subsequently enqueued iterations. */
sbmp_status sbmp_kgmt_set_profiling(sbmp_kgmt* h, int enabled);
/* A 64-bit digest of the replicated planning state after the last enqueued iteration
 * (waits for it): tree rows, region tables of the next iteration, per-iteration control
 * blocks (no reference counterpart).  Every rank of a sharded run holds the same replica,
 * so every rank's digest must be equal: bench.py --gpus N checks it (replicas_agree). */
sbmp_status sbmp_kgmt_state_hash(sbmp_kgmt* h, uint64_t* out);
/* Queue a device-side delay (bounded spin on the GPU clock) so that the
 * launches enqueued after it execute back to back, as in an un-instrumented run. */
sbmp_status sbmp_kgmt_enqueue_delay(sbmp_kgmt* h, double microseconds);
/* Individual launch durations (ms, launch order) of kernel `name` since the last reset. */
sbmp_status sbmp_kgmt_kernel_samples(sbmp_kgmt* h, const char* name, float* out, int capacity, int* count);

/* readObstaclesFromCSV (reference src/helper/helper.cu:11-34): whitespace or
 * comma separated floats, numObstacles = floats / (2*workspaceDim).  Returns
 * SBMP_ERR_IO instead of exit(1) when the file cannot be opened.  capacity is
 * the length of out in floats (>= 2*workspaceDim*numObstacles).  With out == NULL
 * only *numObstacles is computed. */
sbmp_status sbmp_read_obstacles_csv(const char* path, int workspaceDim, float* out, int capacity, int* numObstacles);

/* Legacy random-tree generators behind the reference's Planner interface
 * (include/planners/Planner.cuh:6-12; the reference's CMake does not
 * build them): SBMP_RANDOM_TREE_NAIVE = NaivePlanner::generateRandomTree
 * (NaivePlanner.cu:76-140), SBMP_RANDOM_TREE_COSTPROP = CostPropPlanner
 * (CostPropPlanner.cu:83-139).  rows / blocks / threadsPerBlock <= 0 take the
 * reference's sizes (naive 10 x 32 x 32, costprop 1 x 512 x 1024).  samples: host
 * array of capacity floats >= rows * blocks * threadsPerBlock * 7, row-major like the
 * reference's tree; kernelMs (optional) receives the kernel time.  Semantics and the
 * one deviation (D16): DESIGN.md. */
#define SBMP_RANDOM_TREE_NAIVE 0
#define SBMP_RANDOM_TREE_COSTPROP 1
sbmp_status sbmp_random_tree(int device, int kind, const float* root, int rows, int blocks, int threadsPerBlock,
                             float* samples, long long capacity, float* kernelMs);

/* The uniform-grid obstacle index the planner uses for large obstacle lists
 * (include/sbmp/obstacle_grid.h; replaces the all-boxes loop of isMotionValid,
 * reference src/collisionCheck/collisionCheck.cu:16-28), evaluated on the host:
 * freeOut[i] = isMotionValid(segment i) for nSegments boxes (minx, miny, maxx, maxy).
 * gridSize <= 0 picks the planner's resolution; *gridUsed (optional) receives it.
 * Host-only, no device needed (test entry point). */
sbmp_status sbmp_obstacle_grid_query(const float* obstacles, int nObs, float width, float height, int gridSize,
                                     const float* segments, int nSegments, uint8_t* freeOut, int* gridUsed);

/* ---- Step-level entry points (one stage of the iteration over caller buffers, so each
 * can be parity-tested alone) ----
 *
 * sbmp_expand_batch: propagateG's per-child work (KGMT.cu:386-411): child i expands
 * the parent state parents[7 i .. 7 i + 3] with the XORWOW state rng[6 i .. 6 i + 5]
 * (advanced in place) through propagateAndCheck (include/sbmp/propagator.h, the car;
 * propagatePoint for agent = SBMP_AGENT_POINT), then getR1 / getR2
 * (include/sbmp/grid.h) and, if R1Score and R2Avail are given, the accept test
 * (u <= R1Score[r1] || !R2Avail[r2], one more draw for a valid child; KGMT.cu:394-400).
 * Every pointer is device memory; valid / r1 / r2 / accept may be NULL.
 * sbmp_expand_batch_host runs the same code on the CPU over host buffers. */
typedef struct sbmp_expand_batch_args {
    int count;                       /* children */
    const float* parents;            /* count x 7 */
    uint32_t* rng;                   /* count x 6: v0..v4, d */
    const float* obstacles;          /* obstaclesCount x [xmin, ymin, xmax, ymax] */
    int obstaclesCount;
    int agent;                       /* SBMP_AGENT_CAR / SBMP_AGENT_POINT */
    int numDisc;
    float agentLength, width, height;
    int N, n;                        /* region grid: R1Size = width / N, R2Size = width / (N n) */
    const float* R1Score;            /* N*N, or NULL: no accept test */
    const int* R2Avail;              /* N*N*n*n 0/1 */
    float* children;                 /* count x 7 out: [x, y, theta, v, a, steering, duration] */
    uint8_t* valid;                  /* count out */
    int* r1;                         /* count out (-1: outside the grid) */
    int* r2;                         /* count out */
    uint8_t* accept;                 /* count out */
} sbmp_expand_batch_args;
sbmp_status sbmp_expand_batch(const sbmp_expand_batch_args* args, void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_expand_batch_host(const sbmp_expand_batch_args* args);

/* sbmp_insert_batch: exclusive_scan(GNew) + findInd + updateG (KGMT.cu:221-249,
 * 540-593): the flagged slots, in slot order, become tree rows treeSize + j with
 * parent uParent[slot] and cost = costs[parent] + duration (getCost, KGMT.cu:631-633);
 * min(A, 32 floor(M/32)) rows are written (the updateG grid, KGMT.cu:231), none at or
 * past maxTreeSize (D13); then GNew[0 .. 32 min(A, M/32)) is cleared (D6), all of it
 * with fixGNewClear.  *inserted = A, *goalIndex = the lowest new row within
 * goalThreshold of (goalX, goalY) or -1 (D4).  Device buffers; inserted / goalIndex
 * are device ints. */
typedef struct sbmp_insert_batch_args {
    int slots;
    uint8_t* gnew;                   /* slots: accept flags (cleared as above) */
    const float* unexplored;         /* slots x 7 */
    const int* uParent;              /* slots */
    float* samples;                  /* maxTreeSize x 7 */
    int* parent;                     /* maxTreeSize */
    float* costs;                    /* maxTreeSize */
    int treeSize, maxTreeSize;
    float goalX, goalY, goalThreshold;
    int fixGNewClear;
    int* inserted;                   /* 1 */
    int* goalIndex;                  /* 1 */
} sbmp_insert_batch_args;
sbmp_status sbmp_insert_batch(const sbmp_insert_batch_args* args, void* stream);

/* sbmp_fold_r2_batch: the planner's fold of its R2 key log (k_fold_r2, through the planner's own
 * launcher: its split into workgroups and its LDS opt-in) over a caller ring.  The rule is the
 * host loop of include/sbmp/r2_fold.h: for every iteration t in [tFirst, tLast] with
 * executed[t - tFirst] != 0 and every local key index i < logSlots, the key
 * d_ring[(t % window) * logSlots + i] of global slot (rank + nranks (i / 256)) 256 + i % 256
 * counts iff slot < S[t - tFirst] and (key & 0x7fff) < nR2; it then adds 1 to
 * d_R2Valid[key & 0x7fff] when bit 15 is set, else to d_R2Invalid[key & 0x7fff].  The tables
 * are in/out (nR2 ints each, device memory); 0xffff, 0x7fff and every other cell >= nR2 count
 * nowhere.  d_ring: window x logSlots uint16 in device memory; S, executed: host arrays of
 * tLast - tFirst + 1 ints.  Waits for the result.  SBMP_ERR_INVALID_ARGUMENT for logSlots
 * not a positive multiple of 256, nR2 outside [1, maxR2], tLast - tFirst + 1 outside
 * [1, window], tFirst < 0, tLast >= 2^20, nranks outside [1, maxRanks], rank outside [0, nranks), a NULL
 * buffer.  sbmp_fold_r2_batch_host is that header's loop over host arrays.
 * sbmp_fold_r2_info gives the constants and, for a logSlots (a positive multiple of 256),
 * the launcher's split: `groups` workgroups per iteration, workgroup g taking the keys
 * [g per, min((g + 1) per, logSlots)). */
typedef struct sbmp_fold_info {
    int window;         /* rows of the ring = the most iterations one fold takes (64) */
    int keysPerGroup;   /* the most keys one fold workgroup takes (65,280) */
    int maxR2;          /* the largest nR2 the 16-bit key log serves (32,767) */
    int maxRanks;       /* the largest nranks (8) */
    int groups, per;    /* for logSlots: ceil(logSlots / keysPerGroup), and ceil(logSlots / groups)
                           rounded up to a multiple of 8 */
} sbmp_fold_info;
sbmp_status sbmp_fold_r2_info(int logSlots, sbmp_fold_info* out);
sbmp_status sbmp_fold_r2_batch(const uint16_t* d_ring, const int* S, const int* executed, int tFirst, int tLast,
                               int logSlots, int nR2, int rank, int nranks, int* d_R2Valid, int* d_R2Invalid,
                               void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_fold_r2_batch_host(const uint16_t* ring, const int* S, const int* executed, int tFirst, int tLast,
                                    int logSlots, int nR2, int rank, int nranks, int* R2Valid, int* R2Invalid);

/* sbmp_tree_query_batch: the goal query of sbmp_kgmt_query_goals (k_tree_query) over caller
 * rows: d_state and d_ctrl are device arrays of rows x 4 floats, (x, y, -, -) and
 * (-, -, -, cost), the planner's tree layout; 1 <= rows < 2^31.  goals and out are host
 * arrays of count entries.  Waits for the result.  Errors as sbmp_kgmt_query_goals.
 * sbmp_tree_query_batch_host answers the same over host rows with a plain loop that applies
 * the literal sqrtf(d2) < radius rule to every row (the kernel compares d2 with a
 * threshold): a second statement of the rule, and it needs no device. */
sbmp_status sbmp_tree_query_batch(const float* d_state, const float* d_ctrl, long long rows,
                                  const sbmp_goal_query* goals, int count, sbmp_goal_answer* out,
                                  void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_query_batch_host(const float* state, const float* ctrl, long long rows,
                                       const sbmp_goal_query* goals, int count, sbmp_goal_answer* out);
/* sbmp_tree_query_alive_batch: the masked query of sbmp_kgmt_query_goals_alive (k_tree_query_alive)
 * over caller rows and a caller mask: d_alive holds rows bytes in device memory, and a row is
 * skipped iff its byte is 0 (the rule and the answer over an empty set: sbmp_goal_answer).
 * Everything else, errors included, as sbmp_tree_query_batch; a NULL mask:
 * SBMP_ERR_INVALID_ARGUMENT.  sbmp_tree_query_alive_batch_host is the plain loop of
 * sbmp_tree_query_batch_host with that one test in front, over host rows and a host mask. */
sbmp_status sbmp_tree_query_alive_batch(const float* d_state, const float* d_ctrl, const uint8_t* d_alive,
                                        long long rows, const sbmp_goal_query* goals, int count,
                                        sbmp_goal_answer* out, void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_query_alive_batch_host(const float* state, const float* ctrl, const uint8_t* alive,
                                             long long rows, const sbmp_goal_query* goals, int count,
                                             sbmp_goal_answer* out);
/* sbmp_tree_recheck_batch: the re-check of sbmp_kgmt_recheck_tree (k_tree_recheck, k_tree_alive)
 * over caller rows in the planner's tree layout: state rows x 4 floats (x, y, theta, v), ctrl
 * rows x 4 floats (a, steering, duration, -; a point agent: vx, vy, duration, -), parent rows
 * ints, and obstaclesCount boxes; all four in device memory.  1 <= rows < 2^31; states and
 * controls are finite, a car's steering lies in (-pi, pi] as the planner draws it (D11).  depthBound: an upper bound on the rows of any parent chain (the
 * planner's is its executed iterations + 1), which sets the number of pointer-jumping passes;
 * <= 0: rows, always sufficient because a usable parent is a lower row.  status (host, rows
 * bytes, may be NULL) and *out as sbmp_kgmt_recheck_tree.  Waits for the result.
 * sbmp_tree_recheck_batch_host takes the same arrays in host memory and applies the literal
 * rule in one ascending loop (propagateCarControls / propagatePointControls of
 * include/sbmp/propagator.h): a second statement of the rule, and it needs no device. */
typedef struct sbmp_tree_recheck_args {
    const float* state;
    const float* ctrl;
    const int* parent;
    int rows;
    int depthBound;
    int agent;                /* SBMP_AGENT_* */
    int numDisc;
    float agentLength, width, height;
    const float* obstacles;
    int obstaclesCount;
} sbmp_tree_recheck_args;
sbmp_status sbmp_tree_recheck_batch(const sbmp_tree_recheck_args* args, uint8_t* status, sbmp_tree_recheck* out,
                                    void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_recheck_batch_host(const sbmp_tree_recheck_args* args, uint8_t* status,
                                         sbmp_tree_recheck* out);
/* sbmp_tree_paths_batch / sbmp_tree_trace_batch: sbmp_kgmt_solution_paths (k_path_walk) and
 * sbmp_kgmt_trace_rows (k_tree_trace) over caller rows in the planner's tree layout (state,
 * ctrl, parent as sbmp_tree_recheck_args, in device memory; 1 <= rows < 2^31).  depthBound:
 * the most rows a path may hold; <= 0: rows, always sufficient.
 * sbmp_tree_paths_batch: nodes and every output are host arrays, as sbmp_kgmt_solution_paths.
 * sbmp_tree_trace_batch: d_rows (count ints, or NULL for the rows [0, count)), d_steps
 * (numDisc x count x 4 floats, step-major) and d_status (count bytes) are device memory, so the
 * result can stay on the device; a listed row outside [0, rows) is refused before the launch
 * (the list is read back for that).  Both wait for the result.  The _host twins take every
 * array in host memory and apply the literal rule in plain loops (path_rows_host,
 * trace_rows_host of include/sbmp/tree_paths.h): a second statement of the rule, and they
 * need no device. */
typedef struct sbmp_tree_paths_args {
    const float* state;
    const float* ctrl;
    const int* parent;
    int rows;
    int depthBound;
    int agent;                /* SBMP_AGENT_*; the trace only */
    int numDisc;              /* the trace only */
    float agentLength;        /* the trace only */
} sbmp_tree_paths_args;
sbmp_status sbmp_tree_paths_batch(const sbmp_tree_paths_args* args, const int* nodes, int count, int* lengths,
                                  uint8_t* status, int* rows, float* samples, float* costs, long long capacity,
                                  long long* total, void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_paths_batch_host(const sbmp_tree_paths_args* args, const int* nodes, int count, int* lengths,
                                       uint8_t* status, int* rows, float* samples, float* costs, long long capacity,
                                       long long* total);
sbmp_status sbmp_tree_trace_batch(const sbmp_tree_paths_args* args, const int* d_rows, long long count,
                                  float* d_steps, uint8_t* d_status, void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_trace_batch_host(const sbmp_tree_paths_args* args, const int* rows, long long count,
                                       float* steps, uint8_t* status);
/* sbmp_kgmt_resample_paths over caller rows (args as above; agent, numDisc and agentLength
 * are read).  nodes, counts and status are host arrays; d_states, d_edges and d_times are device
 * memory, so the result can stay on the device.  Waits for the result.  The _host twin takes
 * every array in host memory and applies the literal rule in plain loops (resample_paths_host of
 * include/sbmp/tree_resample.h); it needs no device. */
sbmp_status sbmp_tree_resample_batch(const sbmp_tree_paths_args* args, const int* nodes, int count, double period,
                                     int* counts, uint8_t* status, float* d_states, int* d_edges, double* d_times,
                                     long long capacity, long long* total, void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_resample_batch_host(const sbmp_tree_paths_args* args, const int* nodes, int count, double period,
                                          int* counts, uint8_t* status, float* states, int* edges, double* times,
                                          long long capacity, long long* total);
/* sbmp_tree_extract_batch: the extraction of sbmp_kgmt_extract_tree over caller rows in the
 * planner's tree layout (state, ctrl, parent as sbmp_tree_recheck_args; 1 <= rows < 2^31).
 * depthBound: an upper bound on the rows of any parent chain, which sets the number of
 * pointer-jumping passes; <= 0: rows, always sufficient.  Everything is device memory, so the
 * result can stay there: d_keep (rows bytes, a row is kept iff its byte is non-zero; NULL: every
 * row is kept), d_state, d_ctrl, d_parent and d_origin (`capacity` rows each) and d_newRow (rows
 * ints); each output may be NULL.  *out (host) and the capacity protocol as
 * sbmp_kgmt_extract_tree.  Waits for the result.  The result takes every step-level entry above
 * as it is.  sbmp_tree_extract_batch_host takes the same arrays in host memory and applies the
 * literal rule in plain loops (extract_rows_host of include/sbmp/tree_extract.h): a second
 * statement of the rule, and it needs no device. */
typedef struct sbmp_tree_extract_args {
    const float* state;
    const float* ctrl;
    const int* parent;
    int rows;
    int depthBound;
} sbmp_tree_extract_args;
sbmp_status sbmp_tree_extract_batch(const sbmp_tree_extract_args* args, int root, const uint8_t* d_keep,
                                    float* d_state, float* d_ctrl, int* d_parent, int* d_origin, int* d_newRow,
                                    long long capacity, sbmp_tree_extract* out,
                                    void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_extract_batch_host(const sbmp_tree_extract_args* args, int root, const uint8_t* keep,
                                         float* state, float* ctrl, int* parent, int* origin, int* newRow,
                                         long long capacity, sbmp_tree_extract* out);
/* The launcher's seams (host-only, no device needed): a tile is the rows one workgroup numbers
 * in one go, and the offsets workgroup sums roundTiles tile counts per round.  0 <= rows < 2^31. */
typedef struct sbmp_tree_extract_layout {
    int tileRows;     /* rows per tile (1,024) */
    int roundTiles;   /* tiles the offsets workgroup takes per round (256) */
    int tiles;        /* for rows: ceil(rows / tileRows) */
    int rounds;       /* for rows: ceil(tiles / roundTiles) */
} sbmp_tree_extract_layout;
sbmp_status sbmp_tree_extract_info(long long rows, sbmp_tree_extract_layout* out);
/* sbmp_tree_adopt_tables: the tables an adoption (sbmp_kgmt_adopt_tree) leaves, over caller rows
 * and any grid: k_adopt_scan, k_adopt_seed and k_adopt_tables as the planner launches them.
 * state: device memory, rows x 4.  1 <= rows < 2^31, 0 <= frontierFrom <= rows, width > 0,
 * 1 <= N * N <= 256, 1 <= n <= 16; goal: host, (x, y, radius), or NULL for no disc.  Host outputs,
 * each may be NULL: the five R1 tables of N * N ints, R2bits of ceil(N * N * n * n / 32) words
 * (bit r2 & 31 of word r2 >> 5).  A non-finite frontier row is counted in *out, not refused.
 * Waits for the result.  sbmp_tree_adopt_tables_host takes state in host memory and applies the
 * literal rule in plain loops (adopt_tables_host of include/sbmp/tree_adopt.h). */
typedef struct sbmp_tree_adopt_tables_args {
    const float* state;
    int rows;
    int frontierFrom;
    float width, height;   /* the cells derive from the width (KGMT.cu:13-14) */
    int N, n;
    const float* goal;
} sbmp_tree_adopt_tables_args;
sbmp_status sbmp_tree_adopt_tables(const sbmp_tree_adopt_tables_args* args, int* R1, int* R1Avail, int* R1Valid,
                                   int* R1Invalid, int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out,
                                   void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_adopt_tables_host(const sbmp_tree_adopt_tables_args* args, int* R1, int* R1Avail, int* R1Valid,
                                        int* R1Invalid, int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out);
/* sbmp_tree_reanchor_batch: the re-anchoring of sbmp_kgmt_reanchor_tree (k_reanchor_*) over caller
 * rows in the planner's tree layout; args as for sbmp_tree_recheck_batch, all four arrays in
 * device memory, root = row 0.  newRoot: host, 4 finite floats.  d_outState (rows x 4 floats) and
 * d_alive (rows bytes, 0 / 1) are device memory, so the result can stay there; each may be NULL.
 * status (host, rows bytes, may be NULL) and *out as above.  depthBound: an upper bound on the
 * rows of any parent chain (<= 0: rows, always sufficient), which sets the number of
 * pointer-jumping passes of the depth count.  A bound that is too small is detected and refused
 * with SBMP_ERR_INVALID_ARGUMENT before any row is replayed: a level would read a parent's state
 * before it is written.  Waits for the result.  sbmp_tree_reanchor_batch_host takes the same
 * arrays in host memory (outState and alive included) and applies the literal rule in one
 * ascending loop (reanchor_rows_host of include/sbmp/tree_reanchor.h); it needs no device and
 * does not read depthBound. */
sbmp_status sbmp_tree_reanchor_batch(const sbmp_tree_recheck_args* args, const float newRoot[4], float* d_outState,
                                     uint8_t* d_alive, uint8_t* status, sbmp_tree_reanchor* out,
                                     void* stream /* hipStream_t; NULL: default */);
sbmp_status sbmp_tree_reanchor_batch_host(const sbmp_tree_recheck_args* args, const float newRoot[4], float* outState,
                                          uint8_t* alive, uint8_t* status, sbmp_tree_reanchor* out);

/* The threshold the kernel compares d2 with (host-only, no device needed): *t = the largest
 * float d2 with sqrtf(d2) < r, found by bisecting the float bit patterns with that rule;
 * FLT_MAX for r = +inf; -1 (no d2 is inside) for r <= 0 and for NaN. */
sbmp_status sbmp_goal_radius_threshold(float r, float* t);

/* Device memory helpers replacing demos/main.cu:60-61,64 (cudaMalloc/cudaMemcpy/cudaFree). */
sbmp_status sbmp_device_upload_f32(const float* host, size_t count, float** d_out);
sbmp_status sbmp_device_free(void* d_ptr);
/* Raw device buffers for the step-level entry points: allocate, copy in, copy out. */
sbmp_status sbmp_device_alloc(size_t bytes, void** d_out);
sbmp_status sbmp_device_copy_to(void* d_dst, const void* host, size_t bytes);
sbmp_status sbmp_device_copy_from(void* host, const void* d_src, size_t bytes);
sbmp_status sbmp_device_count(int* count);
/* Measured HBM copy bandwidth of the current device (the STREAM-copy
 * figure quoted next to the 8 TB/s spec): a 16-B-per-lane copy of `bytes` (>= 1 MiB)
 * into a second buffer, best of `reps` passes, GB/s = 2 x bytes / time. */
sbmp_status sbmp_hbm_copy_bandwidth(size_t bytes, int reps, double* gbs);

/* ---- Multi-GPU: one planning problem sharded over ranks (one process per GPU) ----
 * Slots are owned block-cyclically (slot s -> rank (s/256) mod nranks); every
 * rank keeps a full replica of the tree; per iteration the ranks all-reduce one
 * fused exchange buffer over RCCL (region deltas, accept flags and counts) and
 * read each other's accepted children over xGMI (IPC-mapped record buffers), so
 * every rank builds the same tree as a 1-GPU run with the same seed. */
#define SBMP_COMM_ID_BYTES 128
sbmp_status sbmp_comm_get_unique_id(uint8_t id[SBMP_COMM_ID_BYTES]);
sbmp_status sbmp_kgmt_create_sharded(const sbmp_kgmt_params* p, const uint8_t id[SBMP_COMM_ID_BYTES], int nranks,
                                     int rank, sbmp_kgmt** out);
/* The same sharded data flow with nranks ranks on ONE device (p->device) and one
 * stream: the all-reduce is a sum kernel, peer records are read directly.  For
 * testing the sharding on a one-GPU machine; the handle behaves like one planner
 * (exports merge the ranks).  nranks = 1 gives a plain planner. */
sbmp_status sbmp_kgmt_create_local_group(const sbmp_kgmt_params* p, int nranks, sbmp_kgmt** out);

/* ---- Batches: several independent queries on one map, planned together on one GPU ----
 * A batch holds `count` single-GPU planners with one parameter set on one stream.  The
 * members take their own initial states, goals and seeds and share the obstacle list.
 * While every member runs the one-launch form (sbmp_path_info.stepForm), an iteration of
 * all members is one k_step_batch launch, or the fewest launches whose workgroups the
 * device holds at once (a k_step workgroup waits in-kernel for its planner workgroup,
 * so a launch never asks for more than the occupancy query gives; SBMP_BATCH_MAX_GROUPS=n
 * lowers that figure).  Otherwise the members' own launches run in turn.  Every member
 * computes exactly what sbmp_kgmt_plan computes for its query (no reference counterpart:
 * the reference plans one query per KGMT object). */
typedef struct sbmp_kgmt_batch sbmp_kgmt_batch;
typedef struct sbmp_batch_info {
    int count;                /* members */
    int groupsPerMember;      /* 1 + 256-slot blocks: workgroups one member needs resident */
    int residentGroups;       /* k_step_batch workgroups the device holds at once at the last begin
                                 (occupancy x CUs, lowered by SBMP_BATCH_MAX_GROUPS); 0 before it */
    int membersPerLaunch;     /* the most members in one launch (1 when the members run in turn) */
    int launchesPerIteration; /* batch launches per iteration; `count` when the members run in turn */
    int batched;              /* 1: iterations run as k_step_batch launches; 0: the members' own launches
                                 in turn (two-launch form: SBMP_STEP=0, or a member that does not fit) */
} sbmp_batch_info;
/* Fails with SBMP_ERR_INVALID_ARGUMENT for count < 1 or parameters sbmp_kgmt_create rejects. */
sbmp_status sbmp_kgmt_batch_create(const sbmp_kgmt_params* p, int count, sbmp_kgmt_batch** out);
sbmp_status sbmp_kgmt_batch_destroy(sbmp_kgmt_batch* h);
/* initials, goals: host arrays of count x 7 floats; seeds: count; results: count, or NULL.
 * A NULL array or a non-finite root (x, y, theta, v) of any member fails with
 * SBMP_ERR_INVALID_ARGUMENT before anything is launched.  plan blocks until every member has
 * ended (goal, full tree or numIterations); a member's wallMs is taken at its own end.
 * Reuse: as sbmp_kgmt_begin states it, for every member.  batch_begin / batch_plan may be
 * called on a batch in any state (never begun, finished, mid-plan, iterations enqueued and
 * not waited for); every member then computes what a fresh planner would, bit for bit; the
 * obstacle list may change in length and form from call to call (the packing into launches
 * is chosen again at every begin, sbmp_batch_info) and is copied during the call; a
 * member's alive mask does not survive it. */
sbmp_status sbmp_kgmt_batch_plan(sbmp_kgmt_batch* h, const float* initials, const float* goals,
                                 const float* d_obstacles, int obstaclesCount, const uint64_t* seeds,
                                 sbmp_plan_result* results);
sbmp_status sbmp_kgmt_batch_begin(sbmp_kgmt_batch* h, const float* initials, const float* goals,
                                  const float* d_obstacles, int obstaclesCount, const uint64_t* seeds);
/* Up to `iterations` more iterations of every member, waited for; *active = members still running. */
sbmp_status sbmp_kgmt_batch_step(sbmp_kgmt_batch* h, int iterations, int* active);
sbmp_status sbmp_kgmt_batch_enqueue(sbmp_kgmt_batch* h, int iterations);
sbmp_status sbmp_kgmt_batch_sync(sbmp_kgmt_batch* h);
sbmp_status sbmp_kgmt_batch_result(sbmp_kgmt_batch* h, int member, sbmp_plan_result* result);
/* Member i as a planner handle owned by the batch, for every read-only call above
 * (copy_tree, copy_regions, copy_rng, iter_log, solution_path, solution_paths, trace_rows, resample_paths, extract_tree, query_goals, recheck_tree,
 * query_goals_alive, state_hash,
 * export_csv, path_info, kernel_stats, ...).  sbmp_kgmt_plan / begin / step / enqueue / destroy on it fail
 * with SBMP_ERR_STATE, sbmp_kgmt_set_iteration_dump with SBMP_ERR_UNSUPPORTED. */
sbmp_status sbmp_kgmt_batch_member(sbmp_kgmt_batch* h, int i, sbmp_kgmt** borrowed);
sbmp_status sbmp_kgmt_batch_info(sbmp_kgmt_batch* h, sbmp_batch_info* out);
/* The batch launches timed with profileKernels, as kernel "k_step_batch" (the members'
 * own launches are in their sbmp_kgmt_kernel_stats). */
sbmp_status sbmp_kgmt_batch_kernel_stat(sbmp_kgmt_batch* h, sbmp_kernel_stat* out);
/* The packing rule alone (host-only, no device needed): members in index order into the
 * fewest launches whose sum of groupsPerMember stays within residentGroups.
 * launchOfMember[i] = the launch of member i, or -1 if it does not fit alone; *launches =
 * the number of launches. */
sbmp_status sbmp_batch_pack(const int* groupsPerMember, int count, int residentGroups, int* launchOfMember,
                            int* launches);
/* What the planner's constructor decides for a divisor b (host-only, no device needed):
 * *reciprocal = RN(1/b) if the kernels' three-instruction division by b was verified to
 * return RN(a / b) for every mantissa of a, else 0 (the kernels then divide).  The
 * first call for a divisor checks 2^23 quotients (~20 ms); the answer is cached. */
sbmp_status sbmp_division_reciprocal(float b, float* reciprocal);

/* Host collectives for ranks that do not share an RCCL communicator (several
 * processes on one GPU, or a host program that already runs MPI / gloo).  Each
 * callback is collective over the nranks ranks and blocking, on host buffers, and
 * returns 0 on success.  allreduce_*: recv[i] = sum over ranks of send[i];
 * allgather: recv[q * bytes ..] = rank q's `bytes` bytes of send. */
typedef struct sbmp_host_collectives {
    void* ctx;
    int (*allreduce_u64)(void* ctx, const uint64_t* send, uint64_t* recv, size_t count);
    int (*allreduce_i32)(void* ctx, const int32_t* send, int32_t* recv, size_t count);
    int (*allgather)(void* ctx, const void* send, size_t bytes, void* recv);
} sbmp_host_collectives;
/* The sharded planner of sbmp_kgmt_create_sharded (same kernels, k_pack records
 * read over HIP IPC) with its per-iteration all-reduce and the record-buffer
 * handle exchange done by `coll` on the host: the stream is synchronised, the
 * fused buffer copied out, reduced, copied back.  *coll is copied; its callbacks
 * must stay valid until sbmp_kgmt_destroy. */
sbmp_status sbmp_kgmt_create_sharded_host(const sbmp_kgmt_params* p, const sbmp_host_collectives* coll, int nranks,
                                          int rank, sbmp_kgmt** out);

#ifdef __cplusplus
}
#endif

#endif /* SBMP_H */

// kgmt_planner.h — host side of the MI355X KGMT planner (behind the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "kgmt_device.h"
#include "kgmt_launch.h"
#include "sbmp/sbmp.h"

namespace sbmp {

struct Error : std::runtime_error {
    sbmp_status status;
    Error(sbmp_status s, const std::string& m) : std::runtime_error(m), status(s) {}
};

#define SBMP_HIP(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            throw ::sbmp::Error(SBMP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

// Collectives of one rank of a sharded planning problem (kgmt_sharded.cpp: RCCL
// over xGMI, one process per GPU).
class Exchange {
public:
    virtual ~Exchange() = default;
    // recv[i] = sum over ranks of send[i] (stream-ordered, also the per-iteration fence).
    virtual void allreduce_u64(const unsigned long long* send, unsigned long long* recv, size_t n, hipStream_t s) = 0;
    virtual void allreduce_i32(const int* send, int* recv, size_t n, hipStream_t s) = 0;
    // Every rank's device buffer of the same size, mapped into this process (IPC).
    virtual void share_buffer(void* own, size_t bytes, void* peers[kMaxRanks]) = 0;
    // Returns once every rank has called it (host-side; `s` is drained first).  The
    // one-shot exchange waits for its peers in-kernel with a time bound, so ranks are
    // lined up here before their first exchange and after host-side pauses (dumps).
    virtual void barrier(hipStream_t s) = 0;
    virtual int comm_ranks() const { return 0; }   // ranks of the RCCL communicator, 0 if none
};

// What the C ABI drives: one rank (single GPU or one rank of an RCCL group) or a
// local shard group (several ranks on one GPU, used to test the sharded data flow).
class Planner {
public:
    virtual ~Planner() = default;
    virtual void begin(const float* initial, const float* goal, const float* d_obstacles, int nObs, uint64_t seed) = 0;
    virtual void enqueue(int iterations) = 0;
    virtual void sync() = 0;
    virtual void fold_pending() = 0;   // enqueue k_fold_r2 up to the last enqueued iteration
    virtual bool active() = 0;   // syncs; false once the loop has ended
    virtual void rank_barrier() {}   // sharded ranks: all ranks reach this point (Exchange::barrier)
    virtual void result(sbmp_plan_result* r) = 0;
    void run(int pollEvery);     // enqueue until the loop ends
    // plan(): run() with the planner's own loop control (a single k_step rank: the host
    // watches a pinned word instead of polling with stream synchronisations)
    virtual void run_plan() { run(8); }
    // Per-iteration dumps (reference KGMT.cu:263-290, commented out there; read by
    // visualization/visualizationKGMT_Steps.m): with a directory set, run() steps one
    // iteration at a time and writes <dir>/Data/<Kind>/<kind><itr>.csv after each.
    void set_iteration_dump(const std::string& dir) { dumpDir_ = dir; }
    void dump_iteration(const std::string& dir, int itr);

    virtual hipStream_t stream() const = 0;
    virtual int num_slots() const = 0;
    virtual const sbmp_kgmt_params& params() const = 0;

    // exports (reference layouts)
    virtual void copy_tree(float* samples, int* parent, float* costs) = 0;
    virtual void copy_unexplored(float* samples, int* uParent) = 0;
    virtual void copy_flags(uint8_t* G, uint8_t* GNew) = 0;
    virtual void copy_regions(int* R1, int* R1Avail, int* R1Valid, int* R1Invalid, float* R1Score, int* R2Avail,
                              int* R2Valid, int* R2Invalid) = 0;
    virtual void copy_rng(uint32_t* states) = 0;
    virtual std::vector<sbmp_iter_record> iter_log() = 0;
    // Rows root .. node (node < 0: the solution node); returns the length (0: no
    // solution).  Outputs may be null; capacity in rows (too small: SBMP_ERR_INVALID_ARGUMENT).
    virtual int solution_path(int node, int* rows, float* samples, float* costs, int capacity) = 0;
    // Digest of the replicated state (tree rows, region tables, control blocks): the same on
    // every rank of a sharded run (k_state_hash).
    virtual unsigned long long state_hash() = 0;
    // out[i] answers goals[i] over the rows copy_tree exports, [0, min(treeSize, M)), after
    // everything enqueued has finished (k_tree_query; reads the tree only).
    virtual void query_goals(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) = 0;
    // The rows [0, min(treeSize, M)) re-checked against another obstacle list (k_tree_recheck,
    // k_tree_alive; include/sbmp/tree_recheck.h): status is host memory of `capacity` bytes or
    // null; the alive mask stays with the planner until the next begin().  Reads the tree only.
    virtual void recheck_tree(const float* d_obstacles, int nObs, uint8_t* status, int capacity,
                              sbmp_tree_recheck* out) = 0;
    // query_goals over the rows the last recheck_tree left alive.
    virtual void query_goals_alive(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) = 0;
    // Many parent chains and the Euler steps of listed rows over [0, min(treeSize, M)) (k_path_walk,
    // k_tree_trace; include/sbmp/tree_paths.h), as sbmp_kgmt_solution_paths / sbmp_kgmt_trace_rows
    // take them: host arrays, *total set before a capacity error.  They read the tree only.
    virtual void solution_paths(const int* nodes, int count, int* lengths, uint8_t* status, int* rows, float* samples,
                                float* costs, long long capacity, long long* total) = 0;
    virtual void trace_rows(const int* rows, long long count, float* steps, uint8_t* status) = 0;
    // The paths of `count` nodes resampled every `period` seconds (k_resample_clock,
    // k_path_resample; include/sbmp/tree_resample.h), as sbmp_kgmt_resample_paths takes them.
    // Reads the tree only.
    virtual void resample_paths(const int* nodes, int count, double period, int* counts, uint8_t* status, float* states,
                                int* edges, double* times, long long capacity, long long* total) = 0;
    // The subtree below `root` over the kept rows as a tree of its own (k_extract_*;
    // include/sbmp/tree_extract.h), as sbmp_kgmt_extract_tree takes it: host arrays, *out set before
    // a capacity error.  useAlive: the last recheck_tree's mask.  Reads the tree only.
    virtual void extract_tree(int root, bool useAlive, float* state, float* ctrl, int* parent, int* origin, int* newRow,
                              long long capacity, sbmp_tree_extract* out) = 0;
    // A tree adopted as the plan's iteration 1, and the handle's own extracted tree adopted
    // (tree_adopt.hip; include/sbmp/tree_adopt.h), as sbmp_kgmt_adopt_tree / sbmp_kgmt_replan take
    // them.  A single rank only: every other handle refuses (its exchange buffers carry
    // iteration 1's counts by another route).
    virtual void adopt_tree(const sbmp_tree_adopt_args*, const float*, const float*, int, uint64_t, sbmp_tree_adopt*) {
        throw Error(SBMP_ERR_STATE, "adopting a tree is supported on a single-rank planner only, not on a shard group");
    }
    virtual void replan(int, bool, int, const float*, const float*, int, uint64_t, sbmp_tree_adopt*) {
        throw Error(SBMP_ERR_STATE, "replanning by adoption is supported on a single-rank planner only, not on a shard group");
    }
    // The subtree below `root` (every row kept) re-anchored on a measured state (k_reanchor_*;
    // include/sbmp/tree_reanchor.h), as sbmp_kgmt_reanchor_tree takes it: host arrays in the
    // extracted numbering, *out set before a capacity error.  Reads the tree only.
    virtual void reanchor_tree(int root, const float* newRoot, const float* d_obstacles, int nObs, float* state,
                               float* ctrl, int* parent, int* origin, uint8_t* status, long long capacity,
                               sbmp_tree_reanchor* out) = 0;
    // extract, re-anchor, extract the alive rows, adopt: sbmp_kgmt_replan_from.  A single rank only.
    virtual void replan_from(int, const float*, int, const float*, const float*, int, uint64_t, sbmp_tree_reanchor*,
                             sbmp_tree_adopt*) {
        throw Error(SBMP_ERR_STATE, "replanning by adoption is supported on a single-rank planner only, not on a shard group");
    }
    void export_csv(const std::string& dir);

    virtual std::vector<sbmp_kernel_stat> kernel_stats() = 0;
    virtual void path_info(sbmp_path_info* out) = 0;
    virtual void reset_kernel_stats() = 0;
    virtual void set_profiling(bool on) = 0;
    virtual void enqueue_delay(double us) = 0;
    virtual std::vector<float> kernel_samples(const std::string& name) = 0;

protected:
    std::string dumpDir_;
};

// Legacy random-tree generators (random_tree.hip): rows x (blocks * tpb) samples
// of 7 floats into host memory.
void random_tree(int device, int kind, const float* root, int rows, int blocks, int tpb, float* samples,
                 float* kernelMs);

// The passes over a grown tree below share their host-side plumbing: tree_pass.h.
// Goal queries (tree_query.hip; include/sbmp/tree_query.h): the argument checks of every
// entry point, k_tree_query over device rows on `stream` (waits for the result), and the
// literal rule over host rows.
void tree_query_check_goals(const sbmp_goal_query* goals, int count, const sbmp_goal_answer* out);
void tree_query_device(const float* d_state, const float* d_ctrl, long long rows, const sbmp_goal_query* goals,
                       int count, sbmp_goal_answer* out, hipStream_t stream);
// k_tree_query_alive: tree_query_device over the rows whose d_alive byte (tree_recheck_device's mask) is set.
void tree_query_alive_device(const float* d_state, const float* d_ctrl, const uint8_t* d_alive, long long rows,
                             const sbmp_goal_query* goals, int count, sbmp_goal_answer* out, hipStream_t stream);
void tree_query_host(const float* state, const float* ctrl, long long rows, const sbmp_goal_query* goals, int count,
                     sbmp_goal_answer* out);
void tree_query_alive_host(const float* state, const float* ctrl, const uint8_t* alive, long long rows,
                           const sbmp_goal_query* goals, int count, sbmp_goal_answer* out);

// The tree re-check (tree_recheck.hip; include/sbmp/tree_recheck.h).  base: the plan's
// parameters and tree pointers; only a copy with the obstacle fields replaced reaches the
// kernels.  d_alive: `rows` device bytes that receive the alive mask, or null.  status: host,
// `rows` bytes, or null.  Runs on `stream` and waits for the result; scratch is per call.
void tree_recheck_device(const KgmtDev& base, int agent, int variant, int rows, int depthBound,
                         const float* d_obstacles, int nObs, uint8_t* d_alive, uint8_t* status,
                         sbmp_tree_recheck* out, hipStream_t stream);
void tree_recheck_batch(const sbmp_tree_recheck_args* a, uint8_t* status, sbmp_tree_recheck* out, hipStream_t stream);
void tree_recheck_batch_host(const sbmp_tree_recheck_args* a, uint8_t* status, sbmp_tree_recheck* out);

// Paths and traces (tree_paths.hip; include/sbmp/tree_paths.h).  d: the tree pointers and, for
// the trace, numDisc / agentLength and their reciprocals; `rows` rows.  tree_paths_device: nodes
// and every output are host memory (checked by the caller: tree_paths_check); *total is set
// before a capacity error.  tree_trace_device: d_list (or null), d_steps and d_status are
// device memory, the list already checked.  Both run on `stream` and wait for the result.
void tree_paths_check(const int* nodes, int count, int rows, const long long* total);
void tree_paths_device(const KgmtDev& d, int rows, int depthBound, const int* nodes, int count, int* lengths,
                       uint8_t* status, int* outRows, float* samples, float* costs, long long capacity,
                       long long* total, hipStream_t stream);
void tree_trace_check(const int* list, long long count, int rows, const float* steps);
void tree_trace_device(const KgmtDev& d, int agent, int rows, const int* d_list, long long count, float* d_steps,
                       uint8_t* d_status, hipStream_t stream);
// host list and outputs: the device buffers are the call's own
void tree_trace_to_host(const KgmtDev& d, int agent, int rows, const int* list, long long count, float* steps,
                        uint8_t* status, hipStream_t stream);
void tree_paths_batch(const sbmp_tree_paths_args* a, const int* nodes, int count, int* lengths, uint8_t* status,
                      int* rows, float* samples, float* costs, long long capacity, long long* total, hipStream_t stream);
void tree_paths_batch_host(const sbmp_tree_paths_args* a, const int* nodes, int count, int* lengths, uint8_t* status,
                           int* rows, float* samples, float* costs, long long capacity, long long* total);
void tree_trace_batch(const sbmp_tree_paths_args* a, const int* d_rows, long long count, float* d_steps,
                      uint8_t* d_status, hipStream_t stream);
void tree_trace_batch_host(const sbmp_tree_paths_args* a, const int* rows, long long count, float* steps,
                           uint8_t* status);
// k_path_walk's two passes over device arrays, queued on `stream` without a wait (tree_paths.hip):
// pass A writes d_len and d_status, pass B the rows / samples / costs that are non-null at the
// 64-bit row offsets d_off.
void path_walk_lengths_device(const KgmtDev& d, int depthBound, const int* d_nodes, int count, int* d_len,
                              uint8_t* d_status, hipStream_t stream);
void path_walk_rows_device(const KgmtDev& d, int depthBound, const int* d_nodes, int count, int* d_len,
                           uint8_t* d_status, const long long* d_off, int* d_rows, float* d_samples, float* d_costs,
                           hipStream_t stream);

// Paths resampled at a fixed period (tree_resample.hip; include/sbmp/tree_resample.h).  d: the tree
// pointers, numDisc / agentLength and their reciprocals.  nodes, counts and status are host memory;
// states / edges / times are host memory, or device memory with deviceOut set.  *total is set
// before a capacity error.  Runs on `stream` and waits for the result; scratch is per call.
void tree_resample_check(const int* nodes, int count, int rows, double period, const long long* total);
void tree_resample_device(const KgmtDev& d, int agent, int rows, int depthBound, const int* nodes, int count,
                          double period, int* counts, uint8_t* status, float* states, int* edges, double* times,
                          bool deviceOut, long long capacity, long long* total, hipStream_t stream);
void tree_resample_batch(const sbmp_tree_paths_args* a, const int* nodes, int count, double period, int* counts,
                         uint8_t* status, float* d_states, int* d_edges, double* d_times, long long capacity,
                         long long* total, hipStream_t stream);
void tree_resample_batch_host(const sbmp_tree_paths_args* a, const int* nodes, int count, double period, int* counts,
                              uint8_t* status, float* states, int* edges, double* times, long long capacity,
                              long long* total);

// Prune and re-root (tree_extract.hip; include/sbmp/tree_extract.h).  d: the tree pointers; `rows`
// rows, 0 <= root < rows (tree_extract_check_root).  d_keep: rows device bytes, or null (every row
// is kept).  The outputs are host memory, or device memory with deviceOut set; each may be null.
// *out is set before a capacity error.  Runs on `stream` and waits for the result; scratch is per call.
void tree_extract_check_root(int root, int rows);
void tree_extract_device(const KgmtDev& d, int rows, int depthBound, int root, const uint8_t* d_keep, float* state,
                         float* ctrl, int* parent, int* origin, int* newRow, bool deviceOut, long long capacity,
                         sbmp_tree_extract* out, hipStream_t stream);
void tree_extract_batch(const sbmp_tree_extract_args* a, int root, const uint8_t* d_keep, float* d_state, float* d_ctrl,
                        int* d_parent, int* d_origin, int* d_newRow, long long capacity, sbmp_tree_extract* out,
                        hipStream_t stream);
void tree_extract_batch_host(const sbmp_tree_extract_args* a, int root, const uint8_t* keep, float* state, float* ctrl,
                             int* parent, int* origin, int* newRow, long long capacity, sbmp_tree_extract* out);
void tree_extract_info(long long rows, sbmp_tree_extract_layout* out);

// Adoption (tree_adopt.hip; include/sbmp/tree_adopt.h).  d: the planner's grid, goal threshold and
// buffers.  tree_adopt_scan: k_adopt_scan over `rows` device rows with the goal (x, y) given, the
// cells into `scratch` (device, tree_adopt_scratch_bytes(rows)), the summary to the host; it waits
// and writes nothing of the planner's.  tree_adopt_seed: k_adopt_seed and k_adopt_tables queued on
// `stream` behind the plan's clears, without a wait.  The tables pair: the same kernels (or the
// plain loops) over caller rows and any grid, host outputs.
size_t tree_adopt_scratch_bytes(int rows);
void tree_adopt_scan(const KgmtDev& d, const float* d_state, int rows, int frontierFrom, const float* goalXY,
                     void* scratch, sbmp_tree_adopt* out, hipStream_t stream);
void tree_adopt_seed(const KgmtDev& d, const float* d_state, const float* d_ctrl, const int* d_parent, int rows,
                     int frontierFrom, const void* scratch, hipStream_t stream);
void tree_adopt_tables_device(const sbmp_tree_adopt_tables_args* a, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid,
                              int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out, hipStream_t stream);
void tree_adopt_tables_host(const sbmp_tree_adopt_tables_args* a, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid,
                            int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out);

// Re-anchoring (tree_reanchor.hip; include/sbmp/tree_reanchor.h).  base: the plan's parameters
// and the tree pointers (root = row 0); newRoot: host, 4 finite floats; the list and the form as
// for tree_recheck_device.  d_outState (rows x 4) and d_alive (rows bytes): device, or null;
// status: host, or null.  A depthBound below the longest chain is refused (SBMP_ERR_INVALID_ARGUMENT)
// before any row is replayed.  Waits for the result.
void tree_reanchor_device(const KgmtDev& base, int agent, int variant, int rows, int depthBound, const float* newRoot,
                          const float* d_obstacles, int nObs, float* d_outState, uint8_t* d_alive, uint8_t* status,
                          sbmp_tree_reanchor* out, hipStream_t stream);
void tree_reanchor_batch(const sbmp_tree_recheck_args* a, const float* newRoot, float* d_outState, uint8_t* d_alive,
                         uint8_t* status, sbmp_tree_reanchor* out, hipStream_t stream);
void tree_reanchor_batch_host(const sbmp_tree_recheck_args* a, const float* newRoot, float* outState, uint8_t* alive,
                              uint8_t* status, sbmp_tree_reanchor* out);

// Times kernel launches of `ids` kinds with event pairs: the pairs are handed to
// hipExtLaunchKernelGGL, which stamps them with the kernel's own start/end.
class LaunchTimer {
public:
    explicit LaunchTimer(int ids) : launches_(ids, 0), totalMs_(ids, 0.0), samples_(ids) {}
    ~LaunchTimer();
    LaunchTimer(const LaunchTimer&) = delete;
    LaunchTimer& operator=(const LaunchTimer&) = delete;

    KernelTiming take(int id, bool on);   // events for one launch of kind id (a null pair when !on)
    void collect();                       // fold the finished launches into the figures below
    void reset();
    long long launches(int id) const { return launches_[id]; }
    double total_ms(int id) const { return totalMs_[id]; }
    const std::vector<float>& samples(int id) const { return samples_[id]; }

private:
    struct Pending {
        int id;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending_;
    std::vector<hipEvent_t> eventPool_;
    std::vector<long long> launches_;
    std::vector<double> totalMs_;
    std::vector<std::vector<float>> samples_;
};

// The pinned word a single rank's planner workgroups store (KgmtDev::hostPoll).
struct PollWord {
    int seen;   // the last launch whose planner has run
    int end;    // nonzero: that planner found the goal, or its loop ended
};
inline PollWord read_poll_word(const unsigned long long* word) {
    const unsigned long long v = *const_cast<const volatile unsigned long long*>(word);
    return {(int)(v >> 2), (int)(v & 3ull)};
}

class KgmtPlanner : public Planner {
public:
    // nranks > 1: rank `rank` of a sharded problem.  ex = its RCCL collectives, or
    // nullptr inside a LocalShardGroup (which then drives the stages itself);
    // shared = a stream owned by the caller (the group), else the planner makes one.
    KgmtPlanner(const sbmp_kgmt_params& p, int nranks = 1, int rank = 0, Exchange* ex = nullptr,
                hipStream_t shared = nullptr);
    ~KgmtPlanner() override;
    KgmtPlanner(const KgmtPlanner&) = delete;
    KgmtPlanner& operator=(const KgmtPlanner&) = delete;

    // begin()'s checks of one plan's arguments (SBMP_ERR_INVALID_ARGUMENT)
    static void check_begin_args(const float* initial, const float* goal, const float* d_obstacles, int nObs);
    void begin(const float* initial, const float* goal, const float* d_obstacles, int nObs, uint64_t seed) override;
    void enqueue(int iterations) override;
    void sync() override;
    void fold_pending() override {
        if (begun_) fold_to(t_next_ - 1);
    }
    bool active() override;
    void rank_barrier() override {
        if (ex_) ex_->barrier(stream_);
    }
    void result(sbmp_plan_result* r) override;
    void run_plan() override;
    // plan() of `count` single k_step ranks on one stream whose iterations are launched
    // together (one planner, or a BatchGroup's members); see kgmt_planner.cpp.
    //   enqueueOne: launches one more iteration of every member
    //   finish:     the planner's or the group's sync()
    //   raise:      throws member m's wait error e (throw_wait_error, with the caller's wording)
    static void run_to_goal(KgmtPlanner* const* ks, int count, const std::function<void()>& enqueueOne,
                            const std::function<void()>& finish, const std::function<void(int, int)>& raise);

    hipStream_t stream() const override { return stream_; }
    int num_slots() const override { return d_.nSlots; }
    const sbmp_kgmt_params& params() const override { return p_; }

    void copy_tree(float* samples, int* parent, float* costs) override;
    void copy_unexplored(float* samples, int* uParent) override;
    void copy_flags(uint8_t* G, uint8_t* GNew) override;
    void copy_regions(int* R1, int* R1Avail, int* R1Valid, int* R1Invalid, float* R1Score, int* R2Avail,
                      int* R2Valid, int* R2Invalid) override;
    void copy_rng(uint32_t* states) override;
    std::vector<sbmp_iter_record> iter_log() override;
    int solution_path(int node, int* rows, float* samples, float* costs, int capacity) override;
    unsigned long long state_hash() override;
    void query_goals(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) override;
    void recheck_tree(const float* d_obstacles, int nObs, uint8_t* status, int capacity,
                      sbmp_tree_recheck* out) override;
    void query_goals_alive(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) override;
    void solution_paths(const int* nodes, int count, int* lengths, uint8_t* status, int* rows, float* samples,
                        float* costs, long long capacity, long long* total) override;
    void trace_rows(const int* rows, long long count, float* steps, uint8_t* status) override;
    void resample_paths(const int* nodes, int count, double period, int* counts, uint8_t* status, float* states,
                        int* edges, double* times, long long capacity, long long* total) override;
    void extract_tree(int root, bool useAlive, float* state, float* ctrl, int* parent, int* origin, int* newRow,
                      long long capacity, sbmp_tree_extract* out) override;
    void adopt_tree(const sbmp_tree_adopt_args* a, const float* goal, const float* d_obstacles, int nObs, uint64_t seed,
                    sbmp_tree_adopt* out) override;
    void replan(int root, bool useAlive, int frontierFrom, const float* goal, const float* d_obstacles, int nObs,
                uint64_t seed, sbmp_tree_adopt* out) override;
    void reanchor_tree(int root, const float* newRoot, const float* d_obstacles, int nObs, float* state, float* ctrl,
                       int* parent, int* origin, uint8_t* status, long long capacity, sbmp_tree_reanchor* out) override;
    void replan_from(int root, const float* newRoot, int frontierFrom, const float* goal, const float* d_obstacles,
                     int nObs, uint64_t seed, sbmp_tree_reanchor* reanchorOut, sbmp_tree_adopt* out) override;

    std::vector<sbmp_kernel_stat> kernel_stats() override;
    void path_info(sbmp_path_info* out) override;
    void reset_kernel_stats() override;
    void set_profiling(bool on) override { p_.profileKernels = on ? 1 : 0; }
    void enqueue_delay(double us) override { launch_delay(us, stream_); }
    std::vector<float> kernel_samples(const std::string& name) override;

    // ---- stages of one iteration (enqueue() composes them; a LocalShardGroup
    // interleaves them across its ranks)
    int take_iteration();                 // next iteration number, 0 past numIterations
    void stage_expand(int t);
    void stage_pack(int t);               // sharded ranks only
    void stage_exchange(int t);           // sharded ranks with an Exchange: the all-reduce of t
    void stage_finish(int t);
    void stage_fold(int t);               // every kFoldEvery iterations
    void stage_step(int t);               // k_step mode: the iteration's one launch
    void flush();                         // k_step mode: insert the last iteration, plan the next
    bool step_mode() const { return d_.stepMode != 0; }
    // what iteration t sends (sharded k_step alternates two buffers by parity)
    unsigned long long* exchange_send(int t = 0) const { return (t & 1) ? xSendOdd_ : xSend_; }
    unsigned long long* exchange_recv() const { return xRecv_; }
    size_t exchange_words() const { return xWords_; }
    float4* record_buffer() const { return d_.recOut; }
    void set_peer_records(int q, const float4* p) { d_.recPeer[q] = p; }
    void copy_r2_partial(int* R2Valid, int* R2Invalid);   // this rank's folded R2 counters
    int rank() const { return d_.rank; }

private:
    friend class BatchGroup;   // drives its members' k_step launches as one k_step_batch (kgmt_batch.cpp)
    enum KernelId { K_EXPAND = 0, K_FINISH, K_FOLD, K_PACK, K_STEP, K_XCHG, K_COUNT };
    KernelTiming timing(int id) { return timer_.take(id, p_.profileKernels != 0); }
    void read_ctrl(std::vector<IterCtrl>& c, PlannerStatus& st);
    int last_executed(const std::vector<IterCtrl>& c) const;
    void fold_to(int tLast);
    template <typename T>
    T* alloc(size_t n);

    sbmp_kgmt_params p_;
    KgmtDev d_{};
    KgmtDev* dDev_ = nullptr;      // the copy k_step reads (d_.devSelf)
    KgmtDev* dStage_ = nullptr;    // pinned: what was last copied there
    bool uploaded_ = false;
    void upload_dev();
    hipStream_t stream_ = nullptr;
    bool ownStream_ = true;
    Exchange* ex_ = nullptr;
    int t_next_ = 1;
    bool begun_ = false;
    int slotsPadded_ = 0, expandBlocks_ = 0, nbits_ = 1;
    int expandVariant_ = 0;   // SBMP_EXPAND_VARIANT: obstacle form, 0 = auto (3 if <= kMaxRegObs boxes, else 1)
    bool timelineDumped_ = false;
    // Pinned host copy of (ctrl[t_next], status) for active(): both land with one
    // stream synchronisation instead of two blocking copies per poll.
    struct PollBuf {
        IterCtrl ctrl;
        PlannerStatus status;
        unsigned long long word;   // KgmtDev::hostPoll (single rank)
    };
    PollBuf* poll_ = nullptr;
    bool wallFixed_ = false;              // wallMs_ was taken at the goal iteration's end
    bool flushed_ = true;     // k_step mode: the last enqueued iteration has been inserted
    int lastFolded_ = 0;      // iterations <= lastFolded_ are in R2Valid / R2Invalid
    unsigned long long* local_ = nullptr;   // sharded: the owner's block counts + GNew words
    size_t localWords_ = 0;
    unsigned long long* xSend_ = nullptr;
    unsigned long long* xSendOdd_ = nullptr;   // sharded k_step: the send buffer of odd iterations
    bool shStep_ = false;                      // sharded rank in k_step mode
    bool stepCapable_ = false;                 // k_step buffers exist; begin() decides per plan (d_.stepMode)
    int residentGroups_ = 0, neededGroups_ = 0;   // k_step residency at the last begin()
    bool formLogged_ = false;
    void choose_form(const float* d_obstacles, int nObs);
    // what begin() and adopt_tree() share: the clears, the obstacle list and the form before the
    // seeding, and the host-side state after it (tFirst: the first iteration the loop runs)
    void reset_plan(const float* goal, const float* d_obstacles, int nObs);
    void start_plan(int tFirst);
    int firstIter_ = 1;       // the first iteration the loop runs: 1 after begin(), 2 after an adoption
    int adoptedDepth_ = 1;    // rows of the longest parent chain the plan started from (begin(): the root)
    int depth_bound(int executed) const {
        return (int)std::min<long long>((long long)adoptedDepth_ + executed, 0x7fffffff);
    }
    void build_grid(const float* d_obstacles, int nObs);
    unsigned long long* xRecv_ = nullptr;
    size_t xWords_ = 0;
    bool oneshot_ = false;                   // sharded: the exchange is k_oneshot over IPC-mapped inboxes
    bool oneshot_self_test();                // k_oneshot checked once at construction (all ranks agree)
    bool mirror_self_test();                 // the list mirror checked once at construction (all ranks agree)
    bool fused_self_test();                  // the fused exchange's in-kernel order, likewise
    int oneshotCheck_ = 0, mirrorCheck_ = 0, fusedCheck_ = 0;   // start-up checks: 0 not run, 1 passed, -1 failed (fell back)
    unsigned long long* inbox_[kMaxRanks] = {nullptr};
    bool compactX_ = true;   // sharded k_step: k_oneshot sends the compact form of the exchange
    unsigned long long xSeq_ = 0;            // exchanges so far (the same count on every rank)
    uint32_t* jumps_ = nullptr;
    float4* obs_ = nullptr;
    int obsCap_ = 0;
    int* gridStart_ = nullptr;       // obstacle grid index (kObsGrid)
    size_t gridStartCap_ = 0;
    float4* gridBoxes_ = nullptr;
    size_t gridBoxesCap_ = 0;
    std::vector<void*> allocs_;
    unsigned long long* scratch_ = nullptr;   // 8 device words for small results (state_hash)
    unsigned long long* alloc_scratch_u64();
    int settled_rows(bool wait = true, sbmp_plan_result* r = nullptr);   // what a tree pass covers; syncs
    uint8_t* alive_ = nullptr;   // recheck_tree's alive mask, one byte per row of [0, aliveRows_)
    int aliveCap_ = 0;
    int aliveRows_ = -1;         // -1: no re-check since the last begin()
    double wallMs_ = 0.0;
    double t0_ = 0.0;
    LaunchTimer timer_{K_COUNT};
};

// Several ranks of one sharded problem on ONE device and one stream, exchanging
// through a sum kernel instead of RCCL and reading each other's record buffers
// directly.  Same data flow as the RCCL ranks, so the GPU parity tests can prove
// the sharded planner equal to the single-rank one on a one-GPU machine.
class LocalShardGroup : public Planner {
public:
    LocalShardGroup(const sbmp_kgmt_params& p, int nranks);
    ~LocalShardGroup() override;

    void begin(const float* initial, const float* goal, const float* d_obstacles, int nObs, uint64_t seed) override;
    void enqueue(int iterations) override;
    void sync() override {
        for (KgmtPlanner* k : ranks_) k->flush();   // every rank's flush pass (GNew words live with their owner)
        r0().sync();
    }
    void fold_pending() override {
        for (KgmtPlanner* k : ranks_) k->fold_pending();
    }
    bool active() override {
        for (KgmtPlanner* k : ranks_) k->flush();
        return r0().active();
    }
    void result(sbmp_plan_result* r) override { r0().result(r); }

    hipStream_t stream() const override { return stream_; }
    int num_slots() const override { return ranks_[0]->num_slots(); }
    const sbmp_kgmt_params& params() const override { return ranks_[0]->params(); }

    void copy_tree(float* samples, int* parent, float* costs) override { r0().copy_tree(samples, parent, costs); }
    void copy_unexplored(float* samples, int* uParent) override;
    void copy_flags(uint8_t* G, uint8_t* GNew) override;   // GNew words live with their owner
    void copy_regions(int* R1, int* R1Avail, int* R1Valid, int* R1Invalid, float* R1Score, int* R2Avail,
                      int* R2Valid, int* R2Invalid) override;
    void copy_rng(uint32_t* states) override;
    std::vector<sbmp_iter_record> iter_log() override { return r0().iter_log(); }
    int solution_path(int node, int* rows, float* samples, float* costs, int capacity) override {
        return r0().solution_path(node, rows, samples, costs, capacity);   // every rank holds the whole tree
    }
    unsigned long long state_hash() override;   // every rank's digest; throws if they differ
    void query_goals(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) override {
        sync();
        r0().query_goals(goals, count, out);   // every rank holds the whole tree
    }
    void recheck_tree(const float* d_obstacles, int nObs, uint8_t* status, int capacity,
                      sbmp_tree_recheck* out) override {
        sync();
        r0().recheck_tree(d_obstacles, nObs, status, capacity, out);
    }
    void query_goals_alive(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) override {
        sync();
        r0().query_goals_alive(goals, count, out);
    }
    void solution_paths(const int* nodes, int count, int* lengths, uint8_t* status, int* rows, float* samples,
                        float* costs, long long capacity, long long* total) override {
        sync();
        r0().solution_paths(nodes, count, lengths, status, rows, samples, costs, capacity, total);
    }
    void trace_rows(const int* rows, long long count, float* steps, uint8_t* status) override {
        sync();
        r0().trace_rows(rows, count, steps, status);
    }
    void resample_paths(const int* nodes, int count, double period, int* counts, uint8_t* status, float* states,
                        int* edges, double* times, long long capacity, long long* total) override {
        sync();
        r0().resample_paths(nodes, count, period, counts, status, states, edges, times, capacity, total);
    }
    void extract_tree(int root, bool useAlive, float* state, float* ctrl, int* parent, int* origin, int* newRow,
                      long long capacity, sbmp_tree_extract* out) override {
        sync();
        r0().extract_tree(root, useAlive, state, ctrl, parent, origin, newRow, capacity, out);
    }
    void reanchor_tree(int root, const float* newRoot, const float* d_obstacles, int nObs, float* state, float* ctrl,
                       int* parent, int* origin, uint8_t* status, long long capacity, sbmp_tree_reanchor* out) override {
        sync();
        r0().reanchor_tree(root, newRoot, d_obstacles, nObs, state, ctrl, parent, origin, status, capacity, out);
    }

    std::vector<sbmp_kernel_stat> kernel_stats() override { return r0().kernel_stats(); }
    void path_info(sbmp_path_info* out) override { r0().path_info(out); }
    void reset_kernel_stats() override;
    void set_profiling(bool on) override;
    void enqueue_delay(double us) override { r0().enqueue_delay(us); }
    std::vector<float> kernel_samples(const std::string& name) override { return r0().kernel_samples(name); }

private:
    KgmtPlanner& r0() { return *ranks_[0]; }
    hipStream_t stream_ = nullptr;
    std::vector<KgmtPlanner*> ranks_;
};

// Several independent single-rank plans (one parameter set, one obstacle list; their own
// roots, goals and seeds) on ONE device and one stream, one k_step_batch launch per
// iteration for as many members as the device holds at once.  Each
// member is a whole KgmtPlanner (its own buffers, RNG, control blocks, poll word), so
// every export of a member reads as a single planner's would.
class BatchGroup {
public:
    BatchGroup(const sbmp_kgmt_params& p, int count);
    ~BatchGroup();
    BatchGroup(const BatchGroup&) = delete;
    BatchGroup& operator=(const BatchGroup&) = delete;

    int count() const { return (int)members_.size(); }
    KgmtPlanner& member(int i);
    // initials / goals: count x 7 floats; seeds: count
    void begin(const float* initials, const float* goals, const float* d_obstacles, int nObs, const uint64_t* seeds);
    void enqueue(int iterations);   // every member advances by up to `iterations`
    void sync();                    // flush passes, then the stream
    void fold_pending();
    int active();                   // syncs; members whose loop has not ended
    void run_plan();                // until every member has ended (goal, full tree, numIterations)
    void result(int i, sbmp_plan_result* r);
    void info(sbmp_batch_info* out) const;
    sbmp_kernel_stat kernel_stat();   // "k_step_batch": launches timed with profileKernels
    hipStream_t stream() const { return stream_; }

    // Members in index order into the fewest launches whose workgroups (the sum of the
    // members' groups) stay within residentGroups; launchOfMember[i] = -1 for a member
    // that does not fit alone.  Returns the number of launches.  Host-only.
    static int pack(const int* groupsPerMember, int count, int residentGroups, int* launchOfMember);

private:
    struct Launch {
        int first = 0, members = 0, maxGroups = 0;
        StepBatchRec* dTable = nullptr;   // device, `members` records, written at begin()
        StepBatchRec* stage = nullptr;    // pinned: what was last copied there
    };
    void issue(int t, int expand);        // the batch launches of iteration t (or its flush pass)
    void flush();
    void stage_member(KgmtPlanner* k, int t);   // a member's own launches of iteration t
    void free_launches();

    sbmp_kgmt_params p_;
    hipStream_t stream_ = nullptr;
    std::vector<KgmtPlanner*> members_;
    std::vector<Launch> launches_;
    std::vector<int> launchOf_;
    bool begun_ = false, batched_ = false;
    int residentGroups_ = 0, groupsPerMember_ = 0, membersPerLaunch_ = 0;
    LaunchTimer timer_{1};   // k_step_batch
};

// PlannerStatus::error -> the bounded wait that gave up (throws).
[[noreturn]] void throw_wait_error(int e);

double now_ms();

// RN(1/b) if div_by (kgmt_device.h) was verified for the divisor b, else 0 (sbmp_division_reciprocal).
float markstein_rcp(float b);

}  // namespace sbmp

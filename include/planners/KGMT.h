// KGMT.h — drop-in C++ facade of the reference planner class on top of the C ABI.
//
// Replaces reference include/planners/KGMT.cuh:23-109 for callers such as
// demos/main.cu:30,51,60-64: same constructor
//   KGMT(width, height, N, n, numIterations, maxTreeSize, numDisc, agentLength, goalThreshold)
// (KGMT.cuh:28, KGMT.cu:10-78), same void plan(float* initial, float* goal,
// float* d_obstacles, int obstaclesCount) (KGMT.cuh:31, KGMT.cu:80-317), same
// public result fields treeSize_ / costToGoal_ (KGMT.cuh:36,40) and the same prints
// and CSV dumps (KGMT.cu:100,256-257,295-311).  Header-only, plain C++: the caller
// compiles it with any C++ compiler and links libsbmp.so.
//
// Differences, all deliberate:
//   - errors: every ABI failure prints the cause and exit(1)s, matching the
//     reference's CUDA_ERROR_CHECK (helper.cuh:19-27); the reference's own kernel
//     launches are unchecked;
//   - the RNG seed is time(NULL) converted to unsigned long long exactly as the
//     reference's initCurandStates(..., int seed) (KGMT.cu:111, D1); setSeed() makes
//     it explicit for reproducible runs;
//   - plan() may be called more than once (the reference frees ctor-owned buffers
//     at the end of plan, KGMT.cu:314-316);
//   - "time inside KGMT" is wall time of the device-resident loop, not std::clock
//     CPU time (KGMT.cu:294-295).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <iostream>
#include <vector>

#include "sbmp/sbmp.h"

#define SBMP_CHECK(call)                                                                               \
    do {                                                                                               \
        const sbmp_status s_ = (call);                                                                 \
        if (s_ != SBMP_OK) {                                                                           \
            fprintf(stderr, "%s failed: %s: %s\n", #call, sbmp_status_string(s_), sbmp_last_error());  \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)

class KGMT {
public:
    KGMT() = default;
    KGMT(float width, float height, int N, int n, int numIterations, int maxTreeSize, int numDisc, float agentLength,
         float goalThreshold)
        : numIterations_(numIterations), maxTreeSize_(maxTreeSize), numDisc_(numDisc), treeSize_(0), width_(width),
          height_(height), costToGoal_(0.0f), agentLength_(agentLength), R1Threshold_(0.0f),
          goalThreshold_(goalThreshold) {
        SBMP_CHECK(sbmp_kgmt_default_params(&params_));
        params_.width = width;
        params_.height = height;
        params_.N = N;
        params_.n = n;
        params_.numIterations = numIterations;
        params_.maxTreeSize = maxTreeSize;
        params_.numDisc = numDisc;
        params_.agentLength = agentLength;
        params_.goalThreshold = goalThreshold;
        SBMP_CHECK(sbmp_kgmt_create(&params_, &h_));
    }
    // Build extension: every planner parameter, e.g. from a system file (loadConfig).
    explicit KGMT(const sbmp_kgmt_params& p)
        : numIterations_(p.numIterations), maxTreeSize_(p.maxTreeSize), numDisc_(p.numDisc), treeSize_(0),
          width_(p.width), height_(p.height), costToGoal_(0.0f), agentLength_(p.agentLength), R1Threshold_(0.0f),
          goalThreshold_(p.goalThreshold), params_(p) {
        SBMP_CHECK(sbmp_kgmt_create(&params_, &h_));
    }
    ~KGMT() {
        if (h_) sbmp_kgmt_destroy(h_);
    }
    // systems/*.yaml (the reference hardcodes these in main.cu:19-46).
    static sbmp_system_config loadConfig(const char* path) {
        sbmp_system_config c;
        SBMP_CHECK(sbmp_load_system_config(path, &c));
        return c;
    }
    KGMT(const KGMT&) = delete;
    KGMT& operator=(const KGMT&) = delete;

    // KGMT.cu:80-317.  initial / goal: 7 host floats; d_obstacles: device array of
    // obstaclesCount boxes [xmin, ymin, xmax, ymax].
    void plan(float* initial, float* goal, float* d_obstacles, int obstaclesCount) {
        printf("Goal: %f, %f\n", goal[0], goal[1]);   // KGMT.cu:100
        const uint64_t seed = explicitSeed_ ? seed_ : (uint64_t)(long long)(int)time(NULL);
        SBMP_CHECK(sbmp_kgmt_plan(h_, initial, goal, d_obstacles, obstaclesCount, seed, &result_));
        treeSize_ = result_.treeSize;
        costToGoal_ = result_.costToGoal;
        if (costToGoal_ == 0.0f && treeSize_ >= maxTreeSize_) {   // KGMT.cu:256-257
            printf("Iteration %d, Tree size %d\n", result_.iterations, treeSize_);
            printf("Tree size exceeded maxTreeSize\n");
        }
        std::cout << "time inside KGMT is " << result_.wallMs / 1e3 << std::endl;   // KGMT.cu:294-295
        printf("Iteration %d, Tree size %d\n", result_.iterations, treeSize_);       // KGMT.cu:296
        if (writeCsv_) SBMP_CHECK(sbmp_kgmt_export_csv(h_, "."));                   // KGMT.cu:299-311
    }

    // Build extensions.
    void setSeed(uint64_t seed) {
        seed_ = seed;
        explicitSeed_ = true;
    }
    void setWriteCsv(bool on) { writeCsv_ = on; }
    // The per-iteration Data/<Kind>/<kind><itr>.csv dumps of KGMT.cu:263-290 (commented
    // out in the reference); nullptr: off.
    void dumpIterations(const char* dir) { SBMP_CHECK(sbmp_kgmt_set_iteration_dump(h_, dir)); }
    const sbmp_plan_result& result() const { return result_; }
    // Path root .. solution node: tree rows and their 7-float
    // samples; empty if plan() found no solution.
    void solutionPath(std::vector<int>& rows, std::vector<float>& samples) const {
        int n = 0;
        SBMP_CHECK(sbmp_kgmt_solution_path(h_, -1, nullptr, nullptr, nullptr, 0, &n));
        rows.assign(n, 0);
        samples.assign(7 * (size_t)n, 0.0f);
        if (n) SBMP_CHECK(sbmp_kgmt_solution_path(h_, -1, rows.data(), samples.data(), nullptr, n, &n));
    }
    // Goal discs against the tree as it stands (sbmp_kgmt_query_goals; sbmp/tree_query.h): per
    // goal the rows inside, the lowest of them, the cheapest of them and the nearest row.
    // After plan(), or between steps through handle(); the plan goes on unchanged.
    std::vector<sbmp_goal_answer> queryGoals(const std::vector<sbmp_goal_query>& goals) const {
        std::vector<sbmp_goal_answer> out(goals.size());
        SBMP_CHECK(sbmp_kgmt_query_goals(h_, goals.data(), (int)goals.size(), out.data()));
        return out;
    }
    // The tree as it stands re-checked against another obstacle list in device memory
    // (sbmp_kgmt_recheck_tree; sbmp/tree_recheck.h): one SBMP_ROW_* byte per row into status
    // (resized to the rows covered) and the summary.  The plan and its own list are unchanged.
    sbmp_tree_recheck recheckTree(const float* d_obstacles, int obstaclesCount, std::vector<uint8_t>* status = nullptr) const {
        sbmp_tree_recheck s{};
        if (status) status->assign((size_t)(maxTreeSize_ > 0 ? maxTreeSize_ : 1), 0);
        SBMP_CHECK(sbmp_kgmt_recheck_tree(h_, d_obstacles, obstaclesCount, status ? status->data() : nullptr,
                                          status ? (int)status->size() : 0, &s));
        if (status) status->resize((size_t)s.rows);
        return s;
    }
    // queryGoals over the rows the last recheckTree left alive (sbmp_kgmt_query_goals_alive).
    std::vector<sbmp_goal_answer> queryGoalsAlive(const std::vector<sbmp_goal_query>& goals) const {
        std::vector<sbmp_goal_answer> out(goals.size());
        SBMP_CHECK(sbmp_kgmt_query_goals_alive(h_, goals.data(), (int)goals.size(), out.data()));
        return out;
    }
    // The paths root .. node of many nodes in one device pass (sbmp_kgmt_solution_paths;
    // sbmp/tree_paths.h): lengths and status (SBMP_PATH_*) per request, node -1 for none; rows,
    // samples (7 floats per row) and costs hold the paths one behind the other, path i at the sum
    // of lengths[0 .. i).  Returns the total number of path rows.
    long long solutionPaths(const std::vector<int>& nodes, std::vector<int>& lengths, std::vector<uint8_t>& status,
                            std::vector<int>& rows, std::vector<float>& samples, std::vector<float>* costs = nullptr) const {
        return solutionPathsOf(h_, nodes, lengths, status, rows, samples, costs);
    }
    // The numDisc Euler states of the edge that ends on each listed row, bit for bit what the
    // planner integrated (sbmp_kgmt_trace_rows): steps holds numDisc x rows.size() x 4 floats,
    // step-major (step j of entry i at 4 * (j * rows.size() + i)); status one SBMP_ROW_* byte each.
    void traceRows(const std::vector<int>& rows, std::vector<float>& steps, std::vector<uint8_t>& status) const {
        traceRowsOf(h_, numDisc_, rows, steps, status);
    }
    // The paths of many nodes as set-points on one clock, one every `period` seconds of path time
    // from the root, in one device pass (sbmp_kgmt_resample_paths; sbmp/tree_resample.h): counts and
    // status (SBMP_PATH_*) per request; states (4 floats per sample), edges and times hold the paths
    // one behind the other, path i at the sum of counts[0 .. i).  Returns the number of samples.
    long long resamplePaths(const std::vector<int>& nodes, double period, std::vector<int>& counts,
                            std::vector<uint8_t>& status, std::vector<float>& states, std::vector<int>& edges,
                            std::vector<double>& times) const {
        return resamplePathsOf(h_, nodes, period, counts, status, states, edges, times);
    }
    // The subtree below `root` as a tree of its own, in one device pass (sbmp_kgmt_extract_tree;
    // sbmp/tree_extract.h): the rows whose parent chain reaches `root` through kept rows only
    // (useAlive: the rows the last recheckTree left alive; else every row), numbered densely in
    // their old order.  state and ctrl hold 4 floats per new row, parent -1 for the new root,
    // origin the old row of every new row, newRow the new row of every old one (-1: no member).
    sbmp_tree_extract extractTree(int root, bool useAlive, std::vector<float>& state, std::vector<float>& ctrl,
                                  std::vector<int>& parent, std::vector<int>& origin, std::vector<int>& newRow) const {
        return extractTreeOf(h_, root, useAlive, state, ctrl, parent, origin, newRow);
    }
    // A tree adopted in place of begin() and iteration 1 (sbmp_kgmt_adopt_tree; sbmp/tree_adopt.h):
    // state and ctrl hold 4 floats per row (the cost in ctrl's .w), parent one int, as extractTree
    // returns them.  The frontier is the row range [frontierFrom, rows); depthBound <= 0: rows.
    // The loop goes on with sbmp_kgmt_step on handle().
    sbmp_tree_adopt adoptTree(const std::vector<float>& state, const std::vector<float>& ctrl,
                              const std::vector<int>& parent, const float* goal, const float* d_obstacles,
                              int obstaclesCount, uint64_t seed, int frontierFrom = 0, int depthBound = 0) {
        sbmp_tree_adopt_args a{};
        a.state = state.data();
        a.ctrl = ctrl.data();
        a.parent = parent.data();
        a.rows = (int)parent.size();
        a.frontierFrom = frontierFrom;
        a.depthBound = depthBound;
        a.onDevice = 0;
        sbmp_tree_adopt s{};
        SBMP_CHECK(sbmp_kgmt_adopt_tree(h_, &a, goal, d_obstacles, obstaclesCount, seed, &s));
        return s;
    }
    // The planner's own tree below `root` (useAlive: the rows the last recheckTree left alive)
    // adopted against another goal and obstacle list (sbmp_kgmt_replan).
    sbmp_tree_adopt replan(const float* goal, const float* d_obstacles, int obstaclesCount, uint64_t seed, int root = 0,
                           bool useAlive = false, int frontierFrom = 0) {
        sbmp_tree_adopt s{};
        SBMP_CHECK(sbmp_kgmt_replan(h_, root, useAlive ? 1 : 0, frontierFrom, goal, d_obstacles, obstaclesCount, seed, &s));
        return s;
    }
    // The subtree below `root` re-anchored on the measured state newRoot = (x, y, theta, v)
    // (sbmp_kgmt_reanchor_tree; sbmp/tree_reanchor.h): every row replayed from its parent's new
    // state with its stored controls against d_obstacles.  In extractTree's numbering: state holds
    // the new states (a dead row keeps its stored one), status one SBMP_ROW_* byte per row.
    sbmp_tree_reanchor reanchorTree(int root, const float* newRoot, const float* d_obstacles, int obstaclesCount,
                                    std::vector<float>& state, std::vector<float>& ctrl, std::vector<int>& parent,
                                    std::vector<int>& origin, std::vector<uint8_t>& status) const {
        sbmp_tree_extract ex{};   // the size: every row is kept
        SBMP_CHECK(sbmp_kgmt_extract_tree(h_, root, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &ex));
        state.assign(4 * (size_t)ex.kept, 0.0f);
        ctrl.assign(4 * (size_t)ex.kept, 0.0f);
        parent.assign((size_t)ex.kept, 0);
        origin.assign((size_t)ex.kept, 0);
        status.assign((size_t)ex.kept, 0);
        sbmp_tree_reanchor s{};
        SBMP_CHECK(sbmp_kgmt_reanchor_tree(h_, root, newRoot, d_obstacles, obstaclesCount, state.data(), ctrl.data(),
                                           parent.data(), origin.data(), status.data(), ex.kept, &s));
        return s;
    }
    // reanchorTree of the planner's own tree, the rows that stay alive extracted and adopted against
    // `goal` and d_obstacles, all on the device (sbmp_kgmt_replan_from).  reanchored, if given,
    // receives the re-anchoring's summary.
    sbmp_tree_adopt replanFrom(const float* newRoot, const float* goal, const float* d_obstacles, int obstaclesCount,
                               uint64_t seed, int root = 0, int frontierFrom = 0,
                               sbmp_tree_reanchor* reanchored = nullptr) {
        sbmp_tree_adopt s{};
        SBMP_CHECK(sbmp_kgmt_replan_from(h_, root, newRoot, frontierFrom, goal, d_obstacles, obstaclesCount, seed,
                                         reanchored, &s));
        return s;
    }
    // The two calls on any planner handle (KGMTBatch passes a member's).
    static sbmp_tree_extract extractTreeOf(sbmp_kgmt* h, int root, bool useAlive, std::vector<float>& state,
                                           std::vector<float>& ctrl, std::vector<int>& parent, std::vector<int>& origin,
                                           std::vector<int>& newRow) {
        sbmp_tree_extract s{};
        SBMP_CHECK(sbmp_kgmt_extract_tree(h, root, useAlive ? 1 : 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &s));
        state.assign(4 * (size_t)s.kept, 0.0f);
        ctrl.assign(4 * (size_t)s.kept, 0.0f);
        parent.assign((size_t)s.kept, 0);
        origin.assign((size_t)s.kept, 0);
        newRow.assign((size_t)s.rows, -1);
        SBMP_CHECK(sbmp_kgmt_extract_tree(h, root, useAlive ? 1 : 0, state.data(), ctrl.data(), parent.data(),
                                          origin.data(), newRow.data(), s.kept, &s));
        return s;
    }
    static long long solutionPathsOf(sbmp_kgmt* h, const std::vector<int>& nodes, std::vector<int>& lengths,
                                     std::vector<uint8_t>& status, std::vector<int>& rows, std::vector<float>& samples,
                                     std::vector<float>* costs) {
        const int count = (int)nodes.size();
        long long total = 0;
        lengths.assign(nodes.size(), 0);
        status.assign(nodes.size(), 0);
        SBMP_CHECK(sbmp_kgmt_solution_paths(h, nodes.data(), count, lengths.data(), status.data(), nullptr, nullptr,
                                            nullptr, 0, &total));
        rows.assign((size_t)total, 0);
        samples.assign(7 * (size_t)total, 0.0f);
        if (costs) costs->assign((size_t)total, 0.0f);
        if (total)
            SBMP_CHECK(sbmp_kgmt_solution_paths(h, nodes.data(), count, lengths.data(), status.data(), rows.data(),
                                                samples.data(), costs ? costs->data() : nullptr, total, &total));
        return total;
    }
    static long long resamplePathsOf(sbmp_kgmt* h, const std::vector<int>& nodes, double period, std::vector<int>& counts,
                                     std::vector<uint8_t>& status, std::vector<float>& states, std::vector<int>& edges,
                                     std::vector<double>& times) {
        const int count = (int)nodes.size();
        long long total = 0;
        counts.assign(nodes.size(), 0);
        status.assign(nodes.size(), 0);
        SBMP_CHECK(sbmp_kgmt_resample_paths(h, nodes.data(), count, period, counts.data(), status.data(), nullptr,
                                            nullptr, nullptr, 0, &total));
        states.assign(4 * (size_t)total, 0.0f);
        edges.assign((size_t)total, 0);
        times.assign((size_t)total, 0.0);
        if (total)
            SBMP_CHECK(sbmp_kgmt_resample_paths(h, nodes.data(), count, period, counts.data(), status.data(),
                                                states.data(), edges.data(), times.data(), total, &total));
        return total;
    }
    static void traceRowsOf(sbmp_kgmt* h, int numDisc, const std::vector<int>& rows, std::vector<float>& steps,
                            std::vector<uint8_t>& status) {
        steps.assign(4 * (size_t)numDisc * rows.size(), 0.0f);
        status.assign(rows.size(), 0);
        if (!rows.empty())
            SBMP_CHECK(sbmp_kgmt_trace_rows(h, rows.data(), (long long)rows.size(), steps.data(), status.data()));
    }
    sbmp_kgmt* handle() const { return h_; }

    // Public fields of KGMT.cuh:33-43 that carry meaning outside the class.
    int numIterations_ = 0;
    int maxTreeSize_ = 0;
    int numDisc_ = 0;
    int treeSize_ = 0;
    float width_ = 0.0f;
    float height_ = 0.0f;
    float costToGoal_ = 0.0f;
    float agentLength_ = 0.0f;
    float R1Threshold_ = 0.0f;   // dead in the reference (D12)
    float goalThreshold_ = 0.0f;

private:
    sbmp_kgmt_params params_{};
    sbmp_kgmt* h_ = nullptr;
    uint64_t seed_ = 0;
    bool explicitSeed_ = false;
    bool writeCsv_ = true;
    sbmp_plan_result result_{};
};

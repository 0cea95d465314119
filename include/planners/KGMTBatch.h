// KGMTBatch.h — several independent KGMT queries on one map, planned together on one GPU.
//
// No reference counterpart: the reference plans one query per KGMT object
// (include/planners/KGMT.cuh:23-109).  A batch holds `count` planners with KGMT's
// constructor arguments on one stream; the members take their own initial states, goals
// and seeds and share the obstacle list, and one k_step_batch launch per iteration
// advances as many of them as the device holds at once (sbmp_kgmt_batch_* in
// sbmp/sbmp.h).  Every member computes exactly what KGMT::plan computes
// for its query.  Header-only over the C ABI, in the style of KGMT.h: failures print the
// cause and exit(1).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "planners/KGMT.h"

class KGMTBatch {
public:
    KGMTBatch(int count, float width, float height, int N, int n, int numIterations, int maxTreeSize, int numDisc,
              float agentLength, float goalThreshold)
        : count_(count) {
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
        SBMP_CHECK(sbmp_kgmt_batch_create(&params_, count, &h_));
        results_.resize(count);
    }
    // Every planner parameter, e.g. from a system file (KGMT::loadConfig).
    KGMTBatch(int count, const sbmp_kgmt_params& p) : count_(count), params_(p) {
        SBMP_CHECK(sbmp_kgmt_batch_create(&params_, count, &h_));
        results_.resize(count);
    }
    ~KGMTBatch() {
        if (h_) sbmp_kgmt_batch_destroy(h_);
    }
    KGMTBatch(const KGMTBatch&) = delete;
    KGMTBatch& operator=(const KGMTBatch&) = delete;

    int count() const { return count_; }

    // initials / goals: count x 7 host floats; seeds: count; d_obstacles: device array of
    // obstaclesCount boxes [xmin, ymin, xmax, ymax].  Blocks until every member has ended.
    const std::vector<sbmp_plan_result>& plan(const float* initials, const float* goals, const float* d_obstacles,
                                              int obstaclesCount, const uint64_t* seeds) {
        SBMP_CHECK(sbmp_kgmt_batch_plan(h_, initials, goals, d_obstacles, obstaclesCount, seeds, results_.data()));
        return results_;
    }
    void begin(const float* initials, const float* goals, const float* d_obstacles, int obstaclesCount,
               const uint64_t* seeds) {
        SBMP_CHECK(sbmp_kgmt_batch_begin(h_, initials, goals, d_obstacles, obstaclesCount, seeds));
    }
    // Up to `iterations` more iterations of every member; returns the members still running.
    int step(int iterations = 1) {
        int active = 0;
        SBMP_CHECK(sbmp_kgmt_batch_step(h_, iterations, &active));
        return active;
    }
    void enqueue(int iterations) { SBMP_CHECK(sbmp_kgmt_batch_enqueue(h_, iterations)); }
    void sync() { SBMP_CHECK(sbmp_kgmt_batch_sync(h_)); }
    const sbmp_plan_result& result(int i) {
        SBMP_CHECK(sbmp_kgmt_batch_result(h_, i, &results_.at(i)));
        return results_[i];
    }
    sbmp_batch_info info() const {
        sbmp_batch_info b;
        SBMP_CHECK(sbmp_kgmt_batch_info(h_, &b));
        return b;
    }
    // Member i for the read-only sbmp_kgmt_* calls (copy_tree, iter_log, solution_path,
    // export_csv, ...); owned by the batch.
    sbmp_kgmt* member(int i) const {
        sbmp_kgmt* m = nullptr;
        SBMP_CHECK(sbmp_kgmt_batch_member(h_, i, &m));
        return m;
    }
    // Path root .. solution node of member i; empty if it found no solution.
    void solutionPath(int i, std::vector<int>& rows, std::vector<float>& samples) const {
        sbmp_kgmt* m = member(i);
        int n = 0;
        SBMP_CHECK(sbmp_kgmt_solution_path(m, -1, nullptr, nullptr, nullptr, 0, &n));
        rows.assign(n, 0);
        samples.assign(7 * (size_t)n, 0.0f);
        if (n) SBMP_CHECK(sbmp_kgmt_solution_path(m, -1, rows.data(), samples.data(), nullptr, n, &n));
    }
    // Goal discs against member i's tree (KGMT::queryGoals).
    std::vector<sbmp_goal_answer> queryGoals(int i, const std::vector<sbmp_goal_query>& goals) const {
        std::vector<sbmp_goal_answer> out(goals.size());
        SBMP_CHECK(sbmp_kgmt_query_goals(member(i), goals.data(), (int)goals.size(), out.data()));
        return out;
    }
    // Many paths / the Euler steps of listed rows of member i's tree (KGMT::solutionPaths, traceRows).
    long long solutionPaths(int i, const std::vector<int>& nodes, std::vector<int>& lengths, std::vector<uint8_t>& status,
                            std::vector<int>& rows, std::vector<float>& samples, std::vector<float>* costs = nullptr) const {
        return KGMT::solutionPathsOf(member(i), nodes, lengths, status, rows, samples, costs);
    }
    void traceRows(int i, const std::vector<int>& rows, std::vector<float>& steps, std::vector<uint8_t>& status) const {
        KGMT::traceRowsOf(member(i), params_.numDisc, rows, steps, status);
    }
    // Member i's paths on one clock (KGMT::resamplePaths).
    long long resamplePaths(int i, const std::vector<int>& nodes, double period, std::vector<int>& counts,
                            std::vector<uint8_t>& status, std::vector<float>& states, std::vector<int>& edges,
                            std::vector<double>& times) const {
        return KGMT::resamplePathsOf(member(i), nodes, period, counts, status, states, edges, times);
    }
    // Member i's subtree below `root` as a tree of its own (KGMT::extractTree).
    sbmp_tree_extract extractTree(int i, int root, bool useAlive, std::vector<float>& state, std::vector<float>& ctrl,
                                  std::vector<int>& parent, std::vector<int>& origin, std::vector<int>& newRow) const {
        return KGMT::extractTreeOf(member(i), root, useAlive, state, ctrl, parent, origin, newRow);
    }
    sbmp_kgmt_batch* handle() const { return h_; }

private:
    int count_ = 0;
    sbmp_kgmt_params params_{};
    sbmp_kgmt_batch* h_ = nullptr;
    std::vector<sbmp_plan_result> results_;
};

// tree_paths.h — the output stage of a grown tree, stated once for host and device code:
// the parent chain of a row (its path, root first) and the numDisc Euler states of the edge
// that ends on a row (its trace).  No reference counterpart: the reference keeps the goal
// node's cost only (KGMT.cu:586-591), and its visualisation re-integrates every edge in
// double with numDisc fixed to 10 (visualization/visualizationKGMT_Steps.m:88-131).
//
// Path of a node over the rows [0, R), R = min(treeSize, M): the rows node, parent[node], ...
// down to row 0, reported root first.  A step from row r > 0 goes through
// recheck_parent_usable(parent[r], r) only (include/sbmp/tree_recheck.h): a usable parent is a
// strictly lower row, so the walk ends.  The walk counts the row it stands on, then decides:
//     SBMP_PATH_NONE    node == -1                                           length 0
//     SBMP_PATH_DEEP    the count passed depthBound                          length 0
//     SBMP_PATH_OK      the row is row 0                                     length = the count
//     SBMP_PATH_BROKEN  the row has no usable parent (D6's counted-never-    length 0
//                       written rows hold -1; crafted parents)
// so a chain is DEEP when it holds more than depthBound rows before either end is met.  This is
// stricter than k_solution_path, which stops at any negative parent.
//
// Trace of a row r: numDisc states (x, y, theta, v) and one status byte (SBMP_ROW_*).
//     r == 0                          every step holds treeState[0]; SBMP_ROW_FREE
//     r > 0 without a usable parent   every step holds treeState[r]; SBMP_ROW_ORPHAN; nothing is
//                                     loaded through the parent
//     otherwise                       step j (0-based) is the state after j + 1 Euler steps from
//                                     treeState[parent[r]] under treeCtrl[r].xyz, in the
//                                     propagator's sequence and nothing else (propagator.h:
//                                     dt = duration / numDisc, tan(steering) once, per step x and y
//                                     from the old theta and v, then theta, then v, the same
//                                     fmafs); no workspace test, no boxes, no break: a row that
//                                     is in the tree never broke.  SBMP_ROW_FREE if the last step
//                                     is treeState[r] under recheck_same_state, else SBMP_ROW_STALE.
// The point agent emits (x, y, 0, 0).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "sbmp/sbmp.h"
#include "sbmp/sbmp_math.h"
#include "sbmp/tree_recheck.h"

namespace sbmp {

// propagateCarControls (propagator.h) minus its tests: steps receives numDisc x 4 floats,
// `stride` floats apart (4: one row's steps back to back).
SBMP_HD void traceCarControls(const float* x0, int numDisc, float agentLength, float a, float steering, float duration,
                              float* steps, size_t stride = 4) {
    const float dt = duration / (float)numDisc;
    float x = x0[0], y = x0[1], theta = x0[2], v = x0[3];
    const float tan_steering = tanf_d(steering);
    for (int i = 0; i < numDisc; ++i) {
        float sin_theta, cos_theta;
        sincosf_d(theta, &sin_theta, &cos_theta);
        x = __builtin_fmaf(v * cos_theta, dt, x);
        y = __builtin_fmaf(v * sin_theta, dt, y);
        theta = __builtin_fmaf((v / agentLength) * tan_steering, dt, theta);
        v = __builtin_fmaf(a, dt, v);
        float* o = steps + (size_t)i * stride;
        o[0] = x;
        o[1] = y;
        o[2] = theta;
        o[3] = v;
    }
}

// propagatePointControls minus its tests.
SBMP_HD void tracePointControls(const float* x0, int numDisc, float vx, float vy, float duration, float* steps,
                                size_t stride = 4) {
    const float dt = duration / (float)numDisc;
    float x = x0[0], y = x0[1];
    for (int i = 0; i < numDisc; ++i) {
        x = __builtin_fmaf(vx, dt, x);
        y = __builtin_fmaf(vy, dt, y);
        float* o = steps + (size_t)i * stride;
        o[0] = x;
        o[1] = y;
        o[2] = 0.0f;
        o[3] = 0.0f;
    }
}

// One walk of the rule: the status of `node` and, for SBMP_PATH_OK, the rows on its chain.
// visit(k, row) is called for k = 0 (the node) .. length - 1 (row 0) when `emit` is set; the
// caller runs it only after a first walk has said SBMP_PATH_OK.
template <typename Visit>
SBMP_HD uint8_t path_walk(const int* parent, int node, int depthBound, int* length, bool emit, Visit visit) {
    *length = 0;
    if (node == -1) return SBMP_PATH_NONE;
    int count = 0;
    for (int j = node;;) {
        if (++count > depthBound) return SBMP_PATH_DEEP;
        if (emit) visit(count - 1, j);
        if (j == 0) {
            *length = count;
            return SBMP_PATH_OK;
        }
        const int p = parent[j];
        if (!recheck_parent_usable(p, j)) return SBMP_PATH_BROKEN;
        j = p;
    }
}

// true if every node is -1 or a row of [0, rows).
static inline bool path_nodes_valid(const int* nodes, long long count, int rows) {
    for (long long i = 0; i < count; ++i)
        if (nodes[i] < -1 || nodes[i] >= rows) return false;
    return true;
}

// Plain loops over host rows.  lengths / status: count entries each, may be null; the return
// value is the sum of the lengths.  With `out` set the paths are written one behind the other
// in request order, root first, in solution_path's layout: rows (ints), samples (7 floats per
// row: the state and treeCtrl.xyz) and costs (treeCtrl.w); each may be null.
static inline long long path_rows_host(const float* state, const float* ctrl, const int* parent, int depthBound,
                                       const int* nodes, long long count, int* lengths, uint8_t* status, bool out,
                                       int* rows, float* samples, float* costs) {
    long long total = 0;
    for (long long i = 0; i < count; ++i) {
        int len = 0;
        const uint8_t st = path_walk(parent, nodes[i], depthBound, &len, false, [](int, int) {});
        if (lengths) lengths[i] = len;
        if (status) status[i] = st;
        if (out && len > 0) {
            int unused = 0;
            path_walk(parent, nodes[i], depthBound, &unused, true, [&](int k, int row) {
                const size_t at = (size_t)(total + len - 1 - k);
                if (rows) rows[at] = row;
                if (samples) {
                    for (int q = 0; q < 4; ++q) samples[7 * at + q] = state[4 * (size_t)row + q];
                    for (int q = 0; q < 3; ++q) samples[7 * at + 4 + q] = ctrl[4 * (size_t)row + q];
                }
                if (costs) costs[at] = ctrl[4 * (size_t)row + 3];
            });
        }
        total += len;
    }
    return total;
}

// The trace of `count` rows (list[i], or i when list is null; each a row of the tree) into
// steps, step-major: step j of entry i at steps + 4 * (j * count + i).  status: count bytes.
static inline void trace_rows_host(const float* state, const float* ctrl, const int* parent, int agent, int numDisc,
                                   float agentLength, const int* list, long long count, float* steps,
                                   uint8_t* status) {
    for (long long i = 0; i < count; ++i) {
        const int r = list ? list[i] : (int)i;
        float* o = steps + 4 * (size_t)i;
        const size_t stride = 4 * (size_t)count;
        const int p = parent[r];
        const float* me = state + 4 * (size_t)r;
        if (r == 0 || !recheck_parent_usable(p, r)) {
            for (int j = 0; j < numDisc; ++j)
                for (int q = 0; q < 4; ++q) o[(size_t)j * stride + q] = me[q];
            status[i] = r == 0 ? SBMP_ROW_FREE : SBMP_ROW_ORPHAN;
            continue;
        }
        const float* c = ctrl + 4 * (size_t)r;
        if (agent == SBMP_AGENT_POINT) tracePointControls(state + 4 * (size_t)p, numDisc, c[0], c[1], c[2], o, stride);
        else traceCarControls(state + 4 * (size_t)p, numDisc, agentLength, c[0], c[1], c[2], o, stride);
        const float* e = o + (size_t)(numDisc - 1) * stride;
        status[i] = recheck_same_state(e[0], e[1], e[2], e[3], me[0], me[1], me[2], me[3]) ? SBMP_ROW_FREE : SBMP_ROW_STALE;
    }
}

}  // namespace sbmp

// tree_resample.h — solution paths resampled on one clock, stated once for host and device code
// (builds on tree_paths.h; no reference counterpart: the reference keeps the goal node's cost only).
//
// A request is a node (-1, or a row of [0, R)) and shares `period`, a finite double > 0, with the
// other requests of its call.  Its path rows r_0 = 0, r_1, ..., r_{L-1} = node, root first, and its
// status are path_walk's (tree_paths.h); a request whose status is not SBMP_PATH_OK gets 0 samples.
//
// The clock of an OK path: edge k (1 <= k <= L - 1) enters r_k under treeCtrl[r_k].xyz, d_k =
// treeCtrl[r_k].z, e_k = d_k if d_k > 0 and finite, else 0 (a crafted row with a NaN, infinite,
// zero or negative duration adds no time and is never selected).  T_0 = 0, T_k = T_{k-1} +
// (double)e_k, a double sum accumulated in this order, root first; T = T_{L-1}.
//
// n = (long long)floor(T / period) + 2 samples: the grid points m = 0 .. n - 2 and the end sample
// m = n - 1.  T / period >= 2^31 - 2 fails the whole call.  A path of the root alone has T = 0 and
// n = 2, both samples the root at time 0.
//
// Grid sample m <= n - 2: t = (double)m * period.  k = the smallest index of [1, L - 1] with
// t < T_k; without one (L = 1, or fl(m * period) >= T by rounding) the sample is an end sample.
// Otherwise tau = t - T_{k-1}, dt = d_k / (float)numDisc in float32 (the propagator's own dt), j =
// the largest integer of [0, numDisc - 1] with (double)j * (double)dt <= tau (the product is exact),
// alpha = (float)(tau - (double)j * (double)dt), and the state is treeState[r_{k-1}] after j steps
// of traceCarControls' sequence with dt and one more step of the same four fmafs with alpha in
// place of dt: x and y from the old theta and v, then theta from the old v, then v, tan(steering)
// computed once.  The point agent: x = fmaf(vx, dt, x), y likewise, the partial step with alpha,
// theta = v = 0.  edge = r_k, time = t.
// End sample: treeState[node] as stored, edge = node, time = T.
//
// An Euler step is linear in its step length, so in real arithmetic a grid sample lies on the
// segment between Euler states j and j + 1 of its edge: the segment the expand step swept against
// the boxes.  The rule has no workspace test, no boxes and no status per sample.  Every edge
// starts from its parent's STORED state: a row that the trace calls SBMP_ROW_STALE shows as a
// jump at its edge boundary.  With alpha = 0 the sign of a zero is whatever the fmafs give.
//
// Output, paths one behind the other in request order, path i at the exclusive sum of
// counts[0 .. i): states (4 floats: x, y, theta, v), edges (int) and times (double) per sample.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sbmp/sbmp.h"
#include "sbmp/sbmp_math.h"
#include "sbmp/tree_paths.h"

namespace sbmp {

// T / period at or past this fails the call: n = floor(T / period) + 2 stays below 2^31.
constexpr double kResampleMaxRatio = 2147483646.0;

// e_k of a stored duration.
SBMP_HD double resample_edge_time(float d) { return (d > 0.0f && d <= 3.402823466e+38f) ? (double)d : 0.0; }

// n of a path of total time T, or -1 when T / period >= 2^31 - 2.
SBMP_HD int resample_count(double T, double period) {
    const double q = T / period;
    if (!(q < kResampleMaxRatio)) return -1;
    return (int)((long long)floor(q) + 2);
}

// The smallest k of [1, L - 1] with t < T[k], or L when there is none.  T[0 .. L) ascends
// (weakly) from T[0] = 0 <= t, so a bisection finds it in at most log2(L) + 1 rounds.
SBMP_HD int resample_edge_of(const double* T, int L, double t) {
    int lo = 1, hi = L;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (t < T[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The largest j of [0, numDisc - 1] with (double)j * (double)dt <= tau, for tau >= 0.
SBMP_HD int resample_step_of(double tau, float dt, int numDisc) {
    int j = 0;
    while (j + 1 < numDisc && (double)(j + 1) * (double)dt <= tau) ++j;
    return j;
}

// alpha of step j.
SBMP_HD float resample_alpha(double tau, float dt, int j) { return (float)(tau - (double)j * (double)dt); }

// traceCarControls' sequence: j steps of dt and one of alpha from x0, into out[4].
SBMP_HD void resampleCarState(const float* x0, float agentLength, float a, float steering, float dt, int j, float alpha,
                              float* out) {
    float x = x0[0], y = x0[1], theta = x0[2], v = x0[3];
    const float tan_steering = tanf_d(steering);
    for (int i = 0; i <= j; ++i) {
        const float h = (i < j) ? dt : alpha;
        float sin_theta, cos_theta;
        sincosf_d(theta, &sin_theta, &cos_theta);
        x = __builtin_fmaf(v * cos_theta, h, x);
        y = __builtin_fmaf(v * sin_theta, h, y);
        theta = __builtin_fmaf((v / agentLength) * tan_steering, h, theta);
        v = __builtin_fmaf(a, h, v);
    }
    out[0] = x;
    out[1] = y;
    out[2] = theta;
    out[3] = v;
}

// tracePointControls' likewise.
SBMP_HD void resamplePointState(const float* x0, float vx, float vy, float dt, int j, float alpha, float* out) {
    float x = x0[0], y = x0[1];
    for (int i = 0; i <= j; ++i) {
        const float h = (i < j) ? dt : alpha;
        x = __builtin_fmaf(vx, h, x);
        y = __builtin_fmaf(vy, h, y);
    }
    out[0] = x;
    out[1] = y;
    out[2] = 0.0f;
    out[3] = 0.0f;
}

// true for a period the rule takes: finite and > 0.
static inline bool resample_period_valid(double period) { return period > 0.0 && period <= 1.7976931348623157e308; }

// Plain loops over host rows: the second statement of the rule.  counts / status: count entries
// each, may be null.  Returns the number of samples, or -1 when a path's T / period >= 2^31 - 2
// (nothing is written behind that request then).  With `out` set the samples are written one
// path behind the other in request order; states (4 floats per sample), edges and times may each
// be null.  Every node is -1 or a row of the tree (path_nodes_valid) and period is valid.
static inline long long resample_paths_host(const float* state, const float* ctrl, const int* parent, int depthBound,
                                            int agent, int numDisc, float agentLength, const int* nodes,
                                            long long count, double period, int* counts, uint8_t* status, bool out,
                                            float* states, int* edges, double* times) {
    long long total = 0;
    std::vector<int> rows;
    std::vector<double> T;
    for (long long i = 0; i < count; ++i) {
        int L = 0;
        const uint8_t st = path_walk(parent, nodes[i], depthBound, &L, false, [](int, int) {});
        if (status) status[i] = st;
        if (st != SBMP_PATH_OK) {
            if (counts) counts[i] = 0;
            continue;
        }
        rows.assign((size_t)L, 0);
        T.assign((size_t)L, 0.0);
        int unused = 0;
        path_walk(parent, nodes[i], depthBound, &unused, true, [&](int k, int row) { rows[(size_t)(L - 1 - k)] = row; });
        for (int k = 1; k < L; ++k) T[(size_t)k] = T[(size_t)k - 1] + resample_edge_time(ctrl[4 * (size_t)rows[(size_t)k] + 2]);
        const double end = T[(size_t)L - 1];
        const int n = resample_count(end, period);
        if (n < 0) return -1;
        if (counts) counts[i] = n;
        if (out) {
            for (int m = 0; m < n; ++m) {
                const size_t at = (size_t)(total + m);
                const double t = (double)m * period;
                const int k = (m == n - 1) ? L : resample_edge_of(T.data(), L, t);
                if (k >= L) {
                    if (states)
                        for (int q = 0; q < 4; ++q) states[4 * at + q] = state[4 * (size_t)nodes[i] + q];
                    if (edges) edges[at] = nodes[i];
                    if (times) times[at] = end;
                    continue;
                }
                const int r = rows[(size_t)k];
                const float* c = ctrl + 4 * (size_t)r;
                const float* x0 = state + 4 * (size_t)rows[(size_t)k - 1];
                const double tau = t - T[(size_t)k - 1];
                const float dt = c[2] / (float)numDisc;
                const int j = resample_step_of(tau, dt, numDisc);
                const float alpha = resample_alpha(tau, dt, j);
                if (states) {
                    if (agent == SBMP_AGENT_POINT) resamplePointState(x0, c[0], c[1], dt, j, alpha, states + 4 * at);
                    else resampleCarState(x0, agentLength, c[0], c[1], dt, j, alpha, states + 4 * at);
                }
                if (edges) edges[at] = r;
                if (times) times[at] = t;
            }
        }
        total += n;
    }
    return total;
}

}  // namespace sbmp

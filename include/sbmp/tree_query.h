// tree_query.h — the goal query over a grown tree, stated once for host and device code
// (no reference counterpart: the reference asks its tree one question, whether a new row
// entered the one goal disc of plan(), KGMT.cu:635-638).
//
// For a tree row (x, y, cost) and a goal (gx, gy, r), every operation rounded to float
// and never contracted:
//     dx = x - gx,  dy = y - gy,  d2 = dx * dx + dy * dy              (goal_d2)
//     the row is inside  iff  sqrtf(d2) < r, sqrtf correctly rounded   (goal_inside)
// which is inGoalRegion (include/sbmp/grid.h), the planner's own rule:
// false for every r <= 0 and for a NaN r.
//
// Per goal the answer (sbmp_goal_answer, include/sbmp/sbmp.h) over the rows [0, R) is
//     count                         rows inside
//     firstRow                      the lowest row inside, -1 if none
//     bestRow, bestCost             the inside row of lowest cost, the lowest row on ties;
//                                   -1 and 0 if none
//     nearestRow, nearestDistance   the row of lowest d2 over ALL rows, the lowest row on
//                                   ties, and sqrtf of that d2
// Row 0, the root, is a row like any other.  So firstRow equals plan()'s goalIndex whenever
// the root lies outside the disc (the planner tests only the rows it inserts, D4), and it
// is 0 when the root lies inside.
//
// sqrtf is monotone, so for a finite r > 0 the set {d2 : sqrtf(d2) < r} has a largest
// member t(r), and a row is inside iff d2 <= t(r): goal_radius_threshold finds t on the
// host by bisecting the non-negative float bit patterns with the literal rule, and the
// kernel (csrc/tree_query.hip) compares against it, with no sqrt in its loop.
//
// Minima are taken over integer keys (goal_key): costs and d2 are non-negative floats,
// whose bit patterns order as their values do, and the row in the low word breaks ties
// toward the lowest row.  A minimum of keys does not depend on the order the rows arrive
// in, so the answer is the same bits on every run.  (A NaN d2 or cost, which no tree row
// holds, orders by its bit pattern, above +inf.)
//
// The masked query (k_tree_query_alive, sbmp_tree_query_alive_batch, sbmp_kgmt_query_goals_alive)
// takes one byte per row beside the rows:
//     a row is skipped iff its alive byte is 0; any non-zero byte is alive
//     the rows that remain answer as above, and row numbers stay the tree's own
//     with no alive row the answer is count 0, firstRow -1, bestRow -1, bestCost 0,
//     nearestRow -1, nearestDistance +inf
// The last case is kNoGoalKey left in the nearest key: no row produces that key, because rows
// are below 2^31.  The re-check (tree_recheck.h) writes only 0 and 1, and its root is always
// alive; a caller's mask need not be either.
#pragma once

#include <stdint.h>

#include "sbmp/sbmp.h"
#include "sbmp/sbmp_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

SBMP_HD float goal_d2(float x, float y, float gx, float gy) {
    const float dx = x - gx, dy = y - gy;
    return dx * dx + dy * dy;
}

// The literal rule (D18).
SBMP_HD bool goal_inside(float d2, float r) { return __builtin_sqrtf(d2) < r; }

// (value bits) << 32 | row: the minimum over rows is the lowest value, lowest row on ties.
SBMP_HD uint64_t goal_key(float v, uint32_t row) { return ((uint64_t)f2u(v) << 32) | (uint64_t)row; }
constexpr uint64_t kNoGoalKey = ~0ull;   // no row: above every key of a row

// t(r): the largest d2 with sqrtf(d2) < r, so that goal_inside(d2, r) == (d2 <= t) for
// every d2 (a NaN d2 fails both).  r = +inf gives FLT_MAX (sqrtf(inf) < inf is false);
// r <= 0 and a NaN r give -1, which no d2 satisfies.  Host only: 32 evaluations of the
// literal rule on bit patterns, no arithmetic on r.
static inline float goal_radius_threshold(float r) {
    if (!goal_inside(0.0f, r)) return -1.0f;
    uint32_t lo = 0u, hi = 0x7f800000u;   // inside at lo, outside at hi (sqrtf(inf) = inf)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (goal_inside(u2f(mid), r)) lo = mid;
        else hi = mid;
    }
    return u2f(lo);
}

// The answer of one goal from its accumulators: the inside rows' count, the lowest of them
// (~0u if none), the lowest goal_key(cost, row) among them and the lowest goal_key(d2, row)
// over every row that was not skipped (kNoGoalKey if there was none).  Host only.
static inline sbmp_goal_answer goal_answer_of(unsigned count, unsigned first, unsigned long long best,
                                              unsigned long long nearest) {
    sbmp_goal_answer a;
    a.count = (int)count;
    a.firstRow = count ? (int)first : -1;
    a.bestRow = count ? (int)(uint32_t)best : -1;
    a.bestCost = count ? u2f((uint32_t)(best >> 32)) : 0.0f;
    if (nearest == kNoGoalKey) {   // every row was skipped
        a.nearestRow = -1;
        a.nearestDistance = u2f(0x7f800000u);   // +inf
    } else {
        a.nearestRow = (int)(uint32_t)nearest;
        a.nearestDistance = __builtin_sqrtf(u2f((uint32_t)(nearest >> 32)));
    }
    return a;
}

// The literal rule over host rows, row by row (no threshold): what the kernels must reproduce.
// state, ctrl: rows x 4 floats, (x, y, -, -) and (-, -, -, cost); alive: rows bytes, or null
// for the unmasked query.
static inline void query_rows_host(const float* state, const float* ctrl, const uint8_t* alive, long long rows,
                                   const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) {
    for (int i = 0; i < count; ++i) {
        unsigned n = 0u, first = ~0u;
        unsigned long long best = kNoGoalKey, nearest = kNoGoalKey;
        for (long long row = 0; row < rows; ++row) {
            if (alive && alive[row] == 0) continue;
            const float d2 = goal_d2(state[4 * row], state[4 * row + 1], goals[i].x, goals[i].y);
            const unsigned long long nk = goal_key(d2, (uint32_t)row);
            if (nk < nearest) nearest = nk;
            if (!goal_inside(d2, goals[i].radius)) continue;
            ++n;
            if ((unsigned)row < first) first = (unsigned)row;
            const unsigned long long bk = goal_key(ctrl[4 * row + 3], (uint32_t)row);
            if (bk < best) best = bk;
        }
        out[i] = goal_answer_of(n, first, best, nearest);
    }
}

}  // namespace sbmp

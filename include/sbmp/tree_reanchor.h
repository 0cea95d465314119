// tree_reanchor.h — a grown tree re-anchored on a measured root state, stated once for host and
// device code (no reference counterpart: the reference plans from one exact state and never
// moves its root).  DESIGN.md §5.15.
//
// Every pass over a grown tree assumes the robot sits on a tree row bit for bit.  A robot that
// has driven to a row is a few centimetres and a few hundredths of a radian off it, and from
// there the stored controls trace other segments.  Re-anchoring replays the whole tree from a
// new root state s0 = (x, y, theta, v): every row from its parent's NEW state with the row's
// stored controls ctrl[r].xyz, by the expand step's own Euler loop (tree_recheck.h's replay:
// propagateCarControls / propagatePointControls on the host, car_euler / point_euler on the
// device) against an obstacle list.
//
// Over the rows [0, R), R >= 1, root = row 0, every row gets one status and one output state:
//     row 0                      SBMP_ROW_FREE, alive, out[0] = s0 (no edge, nothing tested)
//     parent[r] not in [0, r)    SBMP_ROW_ORPHAN, dead; nothing is loaded through that parent
//     parent dead                SBMP_ROW_FREE | SBMP_ROW_CUT, dead, not replayed: there is no
//                                state to replay from
//     parent alive               the replay from out[parent[r]]: all numDisc steps valid gives
//                                SBMP_ROW_FREE, alive, out[r] = the replay's end state; else
//                                SBMP_ROW_BLOCKED, dead
//     out[r] = state[r] bit for bit for every dead row
// so only alive rows carry new floats.  Controls, parents and costs stay as they are: a cost is
// the edge's duration summed along the chain (KGMT.cu:631), and the controls do not change.
// There is no STALE status: nothing is compared with the stored state.  A usable parent is a
// lower row (recheck_parent_usable), so one ascending loop is the whole rule on the host
// (reanchor_rows_host); on the device a row's replay waits for its parent's, level by level.
// depth[r] = the edges from r to the top of its chain (row 0 or an orphan, depth 0), and
// levels = 1 + the deepest of them.
#pragma once

#include <stdint.h>

#include <vector>

#include "sbmp/propagator.h"
#include "sbmp/sbmp.h"
#include "sbmp/sbmp_math.h"
#include "sbmp/tree_recheck.h"

namespace sbmp {

SBMP_HD bool reanchor_root_finite(float x, float y, float theta, float v) {
    return finitef(x) && finitef(y) && finitef(theta) && finitef(v);
}

// The status of a row r > 0 with a usable parent, from whether that parent is alive and, if it
// is, the replay's verdict.
SBMP_HD uint8_t reanchor_status(bool parentAlive, bool valid) {
    return !parentAlive ? (uint8_t)(SBMP_ROW_FREE | SBMP_ROW_CUT) : valid ? (uint8_t)SBMP_ROW_FREE : (uint8_t)SBMP_ROW_BLOCKED;
}

// One more row in the summary (firstDead starts at -1, the counts at 0; rows ascending).
static inline void reanchor_count_row(sbmp_tree_reanchor* s, int r, uint8_t status) {
    ++s->rows;
    if (status == SBMP_ROW_FREE) ++s->alive;
    else if (status == SBMP_ROW_ORPHAN) ++s->orphan;
    else if (status == SBMP_ROW_BLOCKED) ++s->blocked;
    else ++s->cut;
    if (status != SBMP_ROW_FREE && s->firstDead < 0) s->firstDead = r;
}

// The literal rule over host rows in one ascending loop (state, ctrl: rows x 4 floats; s0: 4
// finite floats; outState: rows x 4 floats; alive: rows bytes; status: rows bytes or null).
// agent: SBMP_AGENT_*.  outState must not overlap state.
static inline void reanchor_rows_host(const float* state, const float* ctrl, const int* parent, int rows,
                                      const float* s0, int agent, int numDisc, float agentLength, float width,
                                      float height, const float* obstacles, int obstaclesCount, float* outState,
                                      uint8_t* alive, uint8_t* status, sbmp_tree_reanchor* out) {
    sbmp_tree_reanchor s = {0, 0, 0, 0, 0, -1, 0};
    std::vector<int> depth((size_t)rows, 0);
    int deepest = 0;
    for (int r = 0; r < rows; ++r) {
        float* o = outState + 4 * (size_t)r;
        const float* me = state + 4 * (size_t)r;
        uint8_t st = SBMP_ROW_FREE;
        if (r == 0) {
            for (int i = 0; i < 4; ++i) o[i] = s0[i];
        } else {
            const int p = parent[r];
            if (!recheck_parent_usable(p, r)) {
                st = SBMP_ROW_ORPHAN;
            } else {
                depth[(size_t)r] = depth[(size_t)p] + 1;
                if (depth[(size_t)r] > deepest) deepest = depth[(size_t)r];
                bool valid = false;
                float x1[7];
                if (alive[p]) {
                    const float* c = ctrl + 4 * (size_t)r;
                    const float* from = outState + 4 * (size_t)p;
                    valid = (agent == SBMP_AGENT_POINT)
                                ? propagatePointControls(from, x1, numDisc, c[0], c[1], c[2], obstacles, obstaclesCount,
                                                         width, height)
                                : propagateCarControls(from, x1, numDisc, agentLength, c[0], c[1], c[2], obstacles,
                                                       obstaclesCount, width, height);
                }
                st = reanchor_status(alive[p] != 0, valid);
                if (st == SBMP_ROW_FREE)
                    for (int i = 0; i < 4; ++i) o[i] = x1[i];
            }
            if (st != SBMP_ROW_FREE)
                for (int i = 0; i < 4; ++i) o[i] = me[i];
        }
        alive[r] = st == SBMP_ROW_FREE ? 1 : 0;
        if (status) status[r] = st;
        reanchor_count_row(&s, r, st);
    }
    s.levels = 1 + deepest;
    *out = s;
}

}  // namespace sbmp

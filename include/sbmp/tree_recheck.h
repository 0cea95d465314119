// tree_recheck.h — the re-check of a grown tree against another obstacle list, stated once
// for host and device code (no reference counterpart: the reference plans against one list
// and never looks at a row again).
//
// Invariant I1 (tests/test_gpu_parity.py): a tree row r > 0 is exactly what the propagator
// makes of treeState[parent[r]] and the row's own controls treeCtrl[r].xyz = (a, steering,
// duration).  The replay of a row is that propagation and nothing else (statePropagator.cu:
// 22-76): dt = duration / numDisc, tan(steering) through the shared implementation
// (D9-D11), numDisc Euler steps with the break semantics of statePropagator.cu:42-45,61-64
// and isMotionValid's four comparisons per box of the NEW list.  On the host it is
// propagateCarControls / propagatePointControls (include/sbmp/propagator.h); on the device
// car_euler / point_euler (csrc/kgmt_device.h), the expand step's own loop.
//
// Over the rows [0, R), R = min(treeSize, M), every row gets one status, the first match:
//     SBMP_ROW_FREE     r == 0 (the root has no edge); r > 0: the replay runs all numDisc
//                       steps valid and ends on treeState[r] bit for bit
//     SBMP_ROW_ORPHAN   r > 0 and parent[r] is not in [0, r): D6's counted-never-written
//                       rows hold -1.  Nothing is loaded through such a parent.
//     SBMP_ROW_BLOCKED  the replay ends invalid (a box of the new list, or the workspace edge)
//     SBMP_ROW_STALE    the replay stays valid but does not reproduce the stored state
//                       (a D6 stale copy, for example)
//     alive[r] = status[r] == FREE && (r == 0 || alive[parent[r]])
// and the exported byte of a FREE row that is not alive has SBMP_ROW_CUT set.  A usable
// parent is a lower row, so one ascending loop decides alive (recheck_rows_host), and every
// ancestor of an alive row is alive: its solution_path is valid as it stands.
#pragma once

#include <stdint.h>

#include "sbmp/propagator.h"
#include "sbmp/sbmp.h"
#include "sbmp/sbmp_math.h"

namespace sbmp {

SBMP_HD bool recheck_parent_usable(int parent, int r) { return parent >= 0 && parent < r; }

// Bit for bit: -0 is not +0, and a NaN equals only its own pattern.
SBMP_HD bool recheck_same_state(float x, float y, float theta, float v, float sx, float sy, float stheta, float sv) {
    return f2u(x) == f2u(sx) && f2u(y) == f2u(sy) && f2u(theta) == f2u(stheta) && f2u(v) == f2u(sv);
}

// The status of a row r > 0 with a usable parent, from its replay's verdict and end state.
SBMP_HD uint8_t recheck_replayed_status(bool valid, bool same) {
    return !valid ? (uint8_t)SBMP_ROW_BLOCKED : same ? (uint8_t)SBMP_ROW_FREE : (uint8_t)SBMP_ROW_STALE;
}

// The exported byte of a row from its status and whether it is alive.
SBMP_HD uint8_t recheck_export_byte(uint8_t status, bool alive) {
    return (status == SBMP_ROW_FREE && !alive) ? (uint8_t)(SBMP_ROW_FREE | SBMP_ROW_CUT) : status;
}

// One more row in the summary (firstDead starts at -1, the counts at 0; rows ascending).
static inline void recheck_count_row(sbmp_tree_recheck* s, int r, uint8_t exported) {
    ++s->rows;
    if (exported == SBMP_ROW_FREE) ++s->alive;
    else if (exported == SBMP_ROW_ORPHAN) ++s->orphan;
    else if (exported == SBMP_ROW_BLOCKED) ++s->blocked;
    else if (exported == SBMP_ROW_STALE) ++s->stale;
    else ++s->cut;
    if (exported != SBMP_ROW_FREE && s->firstDead < 0) s->firstDead = r;
}

// The literal rule over host rows in one ascending loop (state, ctrl: rows x 4 floats; alive:
// rows bytes of scratch; status: rows bytes or null).  agent: SBMP_AGENT_*.
static inline void recheck_rows_host(const float* state, const float* ctrl, const int* parent, int rows, int agent,
                                     int numDisc, float agentLength, float width, float height,
                                     const float* obstacles, int obstaclesCount, uint8_t* alive, uint8_t* status,
                                     sbmp_tree_recheck* out) {
    sbmp_tree_recheck s = {0, 0, 0, 0, 0, 0, -1};
    for (int r = 0; r < rows; ++r) {
        uint8_t st = SBMP_ROW_FREE;
        bool live = true;
        if (r > 0) {
            const int p = parent[r];
            if (!recheck_parent_usable(p, r)) {
                st = SBMP_ROW_ORPHAN;
            } else {
                const float* c = ctrl + 4 * (size_t)r;
                const float* me = state + 4 * (size_t)r;
                float x1[7];
                const bool valid =
                    (agent == SBMP_AGENT_POINT)
                        ? propagatePointControls(state + 4 * (size_t)p, x1, numDisc, c[0], c[1], c[2], obstacles,
                                                 obstaclesCount, width, height)
                        : propagateCarControls(state + 4 * (size_t)p, x1, numDisc, agentLength, c[0], c[1], c[2],
                                               obstacles, obstaclesCount, width, height);
                st = recheck_replayed_status(valid,
                                             recheck_same_state(x1[0], x1[1], x1[2], x1[3], me[0], me[1], me[2], me[3]));
            }
            live = st == SBMP_ROW_FREE && alive[p];   // an orphan's p is never used: st != FREE
        }
        alive[r] = live ? 1 : 0;
        const uint8_t e = recheck_export_byte(st, live);
        if (status) status[r] = e;
        recheck_count_row(&s, r, e);
    }
    *out = s;
}

}  // namespace sbmp

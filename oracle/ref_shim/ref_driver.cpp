// oracle/ref_shim/ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
//
// C entry points over arrays around the reference's own per-child functions, which
// `make -C oracle ref` compiles unmodified for the host into
// oracle/_ref/libkgmt_ref.so:
//   propagateAndCheck, isMotionValid          statePropagator.cu, collisionCheck.cu
//   getR1, getR2, getCost, inGoalRegion       the tail of KGMT.cu
// Nothing of the reference is restated here: this file only loops over rows.  The
// hdr_* entries run the project's public headers (include/sbmp/grid.h, tree_query.h)
// on the same arrays, so that a test can hold the two side by side.
//
// This file is compiled with -ffp-contract=off: it defines the D9 functions the shim
// routes cosf / sinf / tanf to, and sbmp_math.h is written for that setting.
#include <stdint.h>

#include "sbmp/grid.h"
#include "sbmp/sbmp_math.h"
#include "sbmp/tree_query.h"

#include "statePropagator/statePropagator.cuh"   // the reference's declarations (and the shim)

// The tail of KGMT.cu (KGMT.cuh needs thrust, cub and Eigen, so it is not included).
int getR1(float x, float y, float R1Size, int N);
int getR2(float x, float y, int r1, float R1Size, int N, float R2Size, int n);
float getCost(float* x0, float* x1);
bool inGoalRegion(float* x, float* goal, float r);

float ref_shim_cosf(float x) { return sbmp::cosf_d(x); }
float ref_shim_sinf(float x) { return sbmp::sinf_d(x); }
float ref_shim_tanf(float x) { return sbmp::tanf_d(x); }

static float* mut(const float* p) { return const_cast<float*>(p); }

extern "C" {

// parents n x 7, rng n x 6 (v0 .. v4, d; advanced in place), obstacles count x 4
// -> children n x 7, valid n.
void ref_expand(const float* parents, uint32_t* rng, int n, int numDisc, float agentLength, const float* obstacles,
                int count, float width, float height, float* children, uint8_t* valid) {
    static_assert(sizeof(curandState) == 6 * sizeof(uint32_t), "rng rows are XORWOW states");
    for (int i = 0; i < n; ++i) {
        curandState* st = reinterpret_cast<curandState*>(rng + 6 * (long)i);
        valid[i] = propagateAndCheck(mut(parents + 7 * (long)i), children + 7 * (long)i, numDisc, agentLength, st,
                                     mut(obstacles), count, width, height) ? 1 : 0;
    }
}

// xy n x 2 -> r1, r2.  The caller keeps x / R1Size inside int range (the conversion
// is undefined outside it).
void ref_cells(const float* xy, int n, float R1Size, int N, float R2Size, int nn, int* r1, int* r2) {
    for (int i = 0; i < n; ++i) {
        r1[i] = getR1(xy[2 * (long)i], xy[2 * (long)i + 1], R1Size, N);
        r2[i] = getR2(xy[2 * (long)i], xy[2 * (long)i + 1], r1[i], R1Size, N, R2Size, nn);
    }
}

void ref_goal(const float* xy, int n, const float* goal, float r, uint8_t* inside) {
    for (int i = 0; i < n; ++i) inside[i] = inGoalRegion(mut(xy + 2 * (long)i), mut(goal), r) ? 1 : 0;
}

// x0, x1 n x 7 -> cost n.
void ref_cost(const float* x0, const float* x1, int n, float* cost) {
    for (int i = 0; i < n; ++i) cost[i] = getCost(mut(x0 + 7 * (long)i), mut(x1 + 7 * (long)i));
}

// bbMin, bbMax n x 2 (isMotionValid ignores its two end points) -> valid n.
void ref_motion_valid(const float* bbMin, const float* bbMax, int n, const float* obstacles, int count,
                      uint8_t* valid) {
    for (int i = 0; i < n; ++i) {
        float* lo = mut(bbMin + 2 * (long)i);
        float* hi = mut(bbMax + 2 * (long)i);
        valid[i] = isMotionValid(lo, hi, lo, hi, mut(obstacles), count) ? 1 : 0;
    }
}

// The public headers on the same arrays.
void hdr_cells(const float* xy, int n, float R1Size, int N, float R2Size, int nn, int* r1, int* r2) {
    for (int i = 0; i < n; ++i) {
        r1[i] = sbmp::getR1(xy[2 * (long)i], xy[2 * (long)i + 1], R1Size, N);
        r2[i] = sbmp::getR2(xy[2 * (long)i], xy[2 * (long)i + 1], r1[i], R1Size, N, R2Size, nn);
    }
}

// inside: sbmp::inGoalRegion (grid.h); query: goal_inside(goal_d2(..)) (tree_query.h).
void hdr_goal(const float* xy, int n, const float* goal, float r, uint8_t* inside, uint8_t* query) {
    for (int i = 0; i < n; ++i) {
        inside[i] = sbmp::inGoalRegion(xy + 2 * (long)i, goal, r) ? 1 : 0;
        query[i] = sbmp::goal_inside(sbmp::goal_d2(xy[2 * (long)i], xy[2 * (long)i + 1], goal[0], goal[1]), r) ? 1 : 0;
    }
}

}  // extern "C"

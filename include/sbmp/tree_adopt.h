// tree_adopt.h — a tree adopted into a planner as its iteration 1, stated once for host and
// device code (no reference counterpart: the reference seeds one root row, KGMT.cu:85-97, and
// this is that seeding applied to every adopted row).
//
// Inputs: a tree of R rows in the planner's layout (state R x 4 floats, ctrl R x 4 floats with
// the cost in .w, parent R ints), a frontierFrom in [0, R], the grid (width, N, n) and an
// optional goal disc (x, y, radius).
//
// Every row is seeded as the reference seeds its root:
//     r1 = getR1(x, y), r2 = getR2(x, y, r1)      include/sbmp/grid.h; a cell of -1 is not counted (D3)
//     r1 >= 0:  R1[r1] += 1, R1Valid[r1] += 1, R1Avail[r1] = 1
//     r2 >= 0:  bit r2 of R2Avail is set
//     R1Cov[c]  = the set R2 bits of R1 cell c, bits [c n^2, (c + 1) n^2)
//     R1Invalid = 0
// goalRow = the lowest row for which inGoalRegion (D18) holds, -1 if none or without a disc.
// The frontier is the row range [frontierFrom, R).  The summary counts the rows with a
// non-finite x, y, theta or v (nonFinite), those of them inside the frontier
// (frontierNonFinite: a planner refuses the adoption, D15 extended) and the rows with a cell
// of -1 (outOfGrid: r1 < 0 or r2 < 0).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sbmp/grid.h"
#include "sbmp/sbmp.h"

namespace sbmp {

constexpr int kAdoptMaxR1 = 256;   // N * N cells at most: one R1 cell per lane of a 256-lane workgroup
constexpr int kAdoptMaxN2 = 16;    // n at most

// KGMT.cu:13-14: both sizes derive from the width.
SBMP_HD float adopt_r1_size(float width, int N) { return width / (float)N; }
SBMP_HD float adopt_r2_size(float width, int N, int n) { return width / (float)(n * N); }

SBMP_HD bool adopt_row_finite(float x, float y, float theta, float v) {
    return finitef(x) && finitef(y) && finitef(theta) && finitef(v);
}

// The two cells of a row (KGMT.cu:89-90).
SBMP_HD void adopt_row_cells(float x, float y, float R1Size, int N, float R2Size, int n, int* r1, int* r2) {
    *r1 = getR1(x, y, R1Size, N);
    *r2 = getR2(x, y, *r1, R1Size, N, R2Size, n);
}

SBMP_HD bool adopt_row_out_of_grid(int r1, int r2) { return r1 < 0 || r2 < 0; }

// goal: (x, y, radius), or null for no disc.
SBMP_HD bool adopt_row_in_goal(float x, float y, const float* goal) {
    if (!goal) return false;
    const float p[2] = {x, y};
    return inGoalRegion(p, goal, goal[2]);
}

SBMP_HD bool adopt_row_in_frontier(long long row, long long frontierFrom) { return row >= frontierFrom; }

SBMP_HD int adopt_popcount(uint32_t w) { return __builtin_popcount(w); }

// R1Cov of R1 cell c: the set bits among [c nn, (c + 1) nn) of the R2 bit words.
SBMP_HD int adopt_cell_cov(const uint32_t* bits, int c, int nn) {
    const long long lo = (long long)c * nn, hi = lo + nn - 1;   // inclusive
    int cov = 0;
    for (long long w = lo >> 5; w <= (hi >> 5); ++w) {
        uint32_t m = ~0u;
        if (w == (lo >> 5)) m &= ~0u << (lo & 31);
        if (w == (hi >> 5)) m &= ~0u >> (31 - (hi & 31));
        cov += adopt_popcount(bits[w] & m);
    }
    return cov;
}

SBMP_HD int adopt_r2_words(int N, int n) { return (N * N * n * n + 31) / 32; }

// What iteration 2 reads of "iteration 1" (the planner's IterCtrl, field by field): it ran, left
// treeSize rows of which [gLo, treeSize) are the frontier, and drew, expanded and accepted nothing.
struct AdoptCtrl {
    int run, executed, treeSize, gLo, nG, k, nExp, S, H, A;
};
SBMP_HD AdoptCtrl adopt_ctrl(int rows, int frontierFrom) {
    const AdoptCtrl c = {1, 1, rows, frontierFrom, 0, 0, 0, 0, 0, 0};
    return c;
}

// The literal rule in plain loops.  state: rows x 4 floats.  Each table holds N * N ints,
// R2bits adopt_r2_words(N, n) words; each may be null.  1 <= rows, 0 <= frontierFrom <= rows,
// 1 <= N * N <= kAdoptMaxR1, 1 <= n <= kAdoptMaxN2 (checked by the caller).
static inline void adopt_tables_host(const float* state, long long rows, long long frontierFrom, float width, int N,
                                     int n, const float* goal, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid,
                                     int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out) {
    const int nR1 = N * N, nn = n * n, nW = adopt_r2_words(N, n);
    const float R1Size = adopt_r1_size(width, N), R2Size = adopt_r2_size(width, N, n);
    int count[kAdoptMaxR1];
    uint32_t bits[kAdoptMaxR1 * kAdoptMaxN2 * kAdoptMaxN2 / 32];
    memset(count, 0, sizeof(count));
    memset(bits, 0, sizeof(bits));
    sbmp_tree_adopt s;
    memset(&s, 0, sizeof(s));
    s.rows = (int)rows;
    s.goalRow = -1;
    for (long long r = 0; r < rows; ++r) {
        const float* p = state + 4 * (size_t)r;
        int r1, r2;
        adopt_row_cells(p[0], p[1], R1Size, N, R2Size, n, &r1, &r2);
        if (r1 >= 0) count[r1] += 1;
        if (r2 >= 0) bits[r2 >> 5] |= 1u << (r2 & 31);
        if (!adopt_row_finite(p[0], p[1], p[2], p[3])) {
            s.nonFinite += 1;
            if (adopt_row_in_frontier(r, frontierFrom)) s.frontierNonFinite += 1;
        }
        if (adopt_row_out_of_grid(r1, r2)) s.outOfGrid += 1;
        if (s.goalRow < 0 && adopt_row_in_goal(p[0], p[1], goal)) s.goalRow = (int)r;
    }
    for (int c = 0; c < nR1; ++c) {
        if (R1) R1[c] = count[c];
        if (R1Avail) R1Avail[c] = count[c] > 0 ? 1 : 0;
        if (R1Valid) R1Valid[c] = count[c];
        if (R1Invalid) R1Invalid[c] = 0;
        if (R1Cov) R1Cov[c] = adopt_cell_cov(bits, c, nn);
    }
    if (R2bits) memcpy(R2bits, bits, sizeof(uint32_t) * (size_t)nW);
    s.treeSize = (int)rows;
    s.gLo = (int)frontierFrom;
    if (out) *out = s;
}

}  // namespace sbmp

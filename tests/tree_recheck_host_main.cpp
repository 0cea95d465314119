// The host twin of the tree re-check (include/sbmp/tree_recheck.h) as a stand-alone program,
// for a sanitizer build (tests/test_tree_recheck.py compiles it with -fsanitize=address,undefined
// and runs it once).  A small valid tree in exact-size heap arrays; then every crafted parent
// (-1, the row itself, r + 1, INT_MIN, INT_MAX) on rows 1, 5 and the last: each must come out
// ORPHAN with its subtree CUT, and the parent word must never be used as an index (any such read
// lands outside the arrays, where AddressSanitizer stops the program).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbmp/tree_recheck.h"

namespace {
constexpr int kRows = 64;
const float kBoxes[4] = {15.0f, 15.0f, 16.0f, 16.0f};   // away from every row

int fail(const char* what, int a, int b) {
    std::printf("FAILED: %s (%d, %d)\n", what, a, b);
    return 1;
}
}  // namespace

int main() {
    // row r > 0 hangs below row (r - 1) / 2: a binary tree, every row what the propagator makes
    // of its parent and its controls
    float* state = new float[4 * kRows];
    float* ctrl = new float[4 * kRows];
    int* parent = new int[kRows];
    state[0] = 5.0f, state[1] = 5.0f, state[2] = 0.0f, state[3] = 1.0f;
    ctrl[0] = ctrl[1] = ctrl[2] = ctrl[3] = 0.0f;
    parent[0] = -1;
    for (int r = 1; r < kRows; ++r) {
        const int p = (r - 1) / 2;
        float* c = ctrl + 4 * r;
        c[0] = (r & 1) ? 1.0f : -1.0f;
        c[1] = (r & 2) ? 0.4f : -0.4f;
        c[2] = 0.3f;
        float x1[7];
        if (!sbmp::propagateCarControls(state + 4 * p, x1, 10, 1.0f, c[0], c[1], c[2], kBoxes, 1, 20.0f, 20.0f))
            return fail("the base tree has an invalid row", r, 0);
        for (int k = 0; k < 4; ++k) state[4 * r + k] = x1[k];
        c[3] = ctrl[4 * p + 3] + c[2];
        parent[r] = p;
    }
    uint8_t* alive = new uint8_t[kRows];
    uint8_t* status = new uint8_t[kRows];
    sbmp_tree_recheck s;
    sbmp::recheck_rows_host(state, ctrl, parent, kRows, SBMP_AGENT_CAR, 10, 1.0f, 20.0f, 20.0f, kBoxes, 1, alive, status, &s);
    if (s.alive != kRows || s.firstDead != -1) return fail("the base tree is not all alive", s.alive, s.firstDead);

    const int rows[3] = {1, 5, kRows - 1};
    for (int kind = 0; kind < 5; ++kind) {
        std::vector<int> saved(parent, parent + kRows);
        for (int r : rows) {
            const int crafted[5] = {-1, r, r + 1, INT_MIN, INT_MAX};
            parent[r] = crafted[kind];
        }
        sbmp::recheck_rows_host(state, ctrl, parent, kRows, SBMP_AGENT_CAR, 10, 1.0f, 20.0f, 20.0f, kBoxes, 1, alive, status,
                                &s);
        for (int r : rows)
            if (status[r] != SBMP_ROW_ORPHAN) return fail("a crafted parent is not an orphan", kind, r);
        // the subtrees of rows 1 and 5 in the binary tree: 3, 4, 7 .. 10, ... and 11, 12, 23 .. 26, ...
        for (int r = 2; r < kRows - 1; ++r) {
            if (r == 5) continue;
            bool below = false;
            for (int q = saved[r]; q > 0; q = saved[q]) below |= (q == 1 || q == 5);
            const uint8_t want = below ? (SBMP_ROW_FREE | SBMP_ROW_CUT) : SBMP_ROW_FREE;
            if (status[r] != want) return fail("a row below an orphan is not cut, or another row is", kind, r);
        }
        if (s.orphan != 3 || s.rows != s.alive + s.blocked + s.stale + s.orphan + s.cut || s.firstDead != 1)
            return fail("the summary does not add up", kind, s.orphan);
        for (int r = 0; r < kRows; ++r) parent[r] = saved[r];
    }
    // the point agent's body over the same arrays (its verdicts are not this program's subject)
    sbmp::recheck_rows_host(state, ctrl, parent, kRows, SBMP_AGENT_POINT, 10, 1.0f, 20.0f, 20.0f, kBoxes, 1, alive, status, &s);
    if (s.rows != kRows) return fail("rows", s.rows, kRows);
    delete[] state;
    delete[] ctrl;
    delete[] parent;
    delete[] alive;
    delete[] status;
    std::printf("ok\n");
    return 0;
}

// The host twins of the paths and the trace (include/sbmp/tree_paths.h) as a stand-alone program,
// for a sanitizer build (tests/test_tree_paths.py compiles it with -fsanitize=address,undefined
// and runs it once).  A small valid tree in exact-size heap arrays; every crafted parent (-1, the
// row itself, r + 1, INT_MIN, INT_MAX) on rows 1, 5 and the last: a request on such a row or below
// it must come out SBMP_PATH_BROKEN, its trace SBMP_ROW_ORPHAN, and the parent word must never be
// used as an index (any such read lands outside the arrays, where AddressSanitizer stops the
// program).  Then depthBound at the boundary, with outputs of exactly the total's size.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbmp/tree_paths.h"

namespace {
constexpr int kRows = 64, kDisc = 10;

int fail(const char* what, int a, int b) {
    std::printf("FAILED: %s (%d, %d)\n", what, a, b);
    return 1;
}
}  // namespace

int main() {
    // row r > 0 hangs below row (r - 1) / 2: a binary tree, every row the last step of its trace
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
        float steps[4 * kDisc];
        sbmp::traceCarControls(state + 4 * p, kDisc, 1.0f, c[0], c[1], c[2], steps);
        for (int k = 0; k < 4; ++k) state[4 * r + k] = steps[4 * (kDisc - 1) + k];
        c[3] = ctrl[4 * p + 3] + c[2];
        parent[r] = p;
    }
    int* nodes = new int[kRows];
    for (int r = 0; r < kRows; ++r) nodes[r] = r;
    int* lengths = new int[kRows];
    uint8_t* status = new uint8_t[kRows];
    float* steps = new float[4 * kDisc * kRows];
    uint8_t* rowStatus = new uint8_t[kRows];

    // the whole tree: every path OK, every trace FREE
    long long total = sbmp::path_rows_host(state, ctrl, parent, kRows, nodes, kRows, lengths, status, false, nullptr,
                                           nullptr, nullptr);
    for (int r = 0; r < kRows; ++r)
        if (status[r] != SBMP_PATH_OK || lengths[r] < 1) return fail("the base tree has a bad path", r, status[r]);
    {
        int* rows = new int[total];
        float* samples = new float[7 * total];
        float* costs = new float[total];
        if (sbmp::path_rows_host(state, ctrl, parent, kRows, nodes, kRows, nullptr, nullptr, true, rows, samples, costs) != total)
            return fail("the second walk's total differs", (int)total, 0);
        long long at = 0;
        for (int r = 0; r < kRows; ++r) {
            if (rows[at] != 0 || rows[at + lengths[r] - 1] != r) return fail("a path does not run root .. node", r, rows[at]);
            at += lengths[r];
        }
        delete[] rows;
        delete[] samples;
        delete[] costs;
    }
    sbmp::trace_rows_host(state, ctrl, parent, SBMP_AGENT_CAR, kDisc, 1.0f, nullptr, kRows, steps, rowStatus);
    for (int r = 0; r < kRows; ++r)
        if (rowStatus[r] != SBMP_ROW_FREE) return fail("the base tree has a row that is not free", r, rowStatus[r]);

    const int crafted_rows[3] = {1, 5, kRows - 1};
    for (int kind = 0; kind < 5; ++kind) {
        std::vector<int> saved(parent, parent + kRows);
        for (int r : crafted_rows) {
            const int crafted[5] = {-1, r, r + 1, INT_MIN, INT_MAX};
            parent[r] = crafted[kind];
        }
        sbmp::path_rows_host(state, ctrl, parent, kRows, nodes, kRows, lengths, status, false, nullptr, nullptr, nullptr);
        sbmp::trace_rows_host(state, ctrl, parent, SBMP_AGENT_CAR, kDisc, 1.0f, nodes, kRows, steps, rowStatus);
        for (int r = 0; r < kRows; ++r) {
            bool broken = false, self = false;
            for (int c : crafted_rows) self |= (r == c);
            for (int q = r; q > 0; q = saved[q])
                for (int c : crafted_rows) broken |= (q == c);
            if (status[r] != (broken ? SBMP_PATH_BROKEN : SBMP_PATH_OK)) return fail("path status", kind, r);
            if (broken && lengths[r] != 0) return fail("a broken path has a length", kind, r);
            if (rowStatus[r] != (self ? SBMP_ROW_ORPHAN : SBMP_ROW_FREE)) return fail("trace status", kind, r);
        }
        for (int r = 0; r < kRows; ++r) parent[r] = saved[r];
    }

    // depthBound at the boundary: row 63's chain is 63, 31, 15, 7, 3, 1, 0
    const int last[1] = {kRows - 1};
    int len = 0;
    uint8_t st = 0;
    if (sbmp::path_rows_host(state, ctrl, parent, 7, last, 1, &len, &st, false, nullptr, nullptr, nullptr) != 7 ||
        st != SBMP_PATH_OK || len != 7)
        return fail("depthBound equal to the chain", st, len);
    {
        int* rows = new int[7];
        float* samples = new float[49];
        float* costs = new float[7];
        sbmp::path_rows_host(state, ctrl, parent, 7, last, 1, nullptr, nullptr, true, rows, samples, costs);
        const int want[7] = {0, 1, 3, 7, 15, 31, 63};
        for (int k = 0; k < 7; ++k)
            if (rows[k] != want[k]) return fail("the chain's rows", k, rows[k]);
        delete[] rows;
        delete[] samples;
        delete[] costs;
    }
    if (sbmp::path_rows_host(state, ctrl, parent, 6, last, 1, &len, &st, false, nullptr, nullptr, nullptr) != 0 ||
        st != SBMP_PATH_DEEP || len != 0)
        return fail("depthBound one short of the chain", st, len);
    const int none[1] = {-1};
    if (sbmp::path_rows_host(state, ctrl, parent, 7, none, 1, &len, &st, false, nullptr, nullptr, nullptr) != 0 ||
        st != SBMP_PATH_NONE)
        return fail("node -1", st, len);
    // the point agent's body over the same arrays, one listed row, exact-size output
    {
        float* one = new float[4 * kDisc];
        uint8_t b = 0;
        sbmp::trace_rows_host(state, ctrl, parent, SBMP_AGENT_POINT, kDisc, 1.0f, last, 1, one, &b);
        if (b != SBMP_ROW_STALE) return fail("a car's row under the point's body", b, 0);
        delete[] one;
    }
    delete[] state;
    delete[] ctrl;
    delete[] parent;
    delete[] nodes;
    delete[] lengths;
    delete[] status;
    delete[] steps;
    delete[] rowStatus;
    std::printf("ok\n");
    return 0;
}

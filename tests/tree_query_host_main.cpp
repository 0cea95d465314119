// The host twin of the goal query (include/sbmp/tree_query.h) as a stand-alone program, for a
// sanitizer build (tests/test_tree_query.py compiles it with -fsanitize=address,undefined and runs
// it once).  Rows, mask, goals and answers live in heap arrays sized to the byte, so a read one
// row, one mask byte or one goal past the end stops the program.  Checked: the masked loop over a
// mixed mask, a mask of ones and a null mask against each other, any non-zero byte as alive, the
// all-dead mask's empty-set answer, one alive row at either end, and the one-row tree.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sbmp/tree_query.h"

namespace {
int fail(const char* what, int a, int b) {
    std::printf("FAILED: %s (%d, %d)\n", what, a, b);
    return 1;
}

bool same(const sbmp_goal_answer& a, const sbmp_goal_answer& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

bool empty(const sbmp_goal_answer& a) {
    return a.count == 0 && a.firstRow == -1 && a.bestRow == -1 && sbmp::f2u(a.bestCost) == 0u && a.nearestRow == -1 &&
           sbmp::f2u(a.nearestDistance) == 0x7f800000u;
}
}  // namespace

int main() {
    constexpr int kRows = 517, kGoals = 5;
    float* state = new float[4 * kRows];
    float* ctrl = new float[4 * kRows];
    uint8_t* mask = new uint8_t[kRows];
    sbmp_goal_query* goals = new sbmp_goal_query[kGoals];
    sbmp_goal_answer* out = new sbmp_goal_answer[kGoals];
    sbmp_goal_answer* ref = new sbmp_goal_answer[kGoals];
    // rows on a 23-column lattice of pitch 0.5 from (1, 1); cost falls with the row
    for (int r = 0; r < kRows; ++r) {
        state[4 * r] = 1.0f + 0.5f * (float)(r % 23);
        state[4 * r + 1] = 1.0f + 0.5f * (float)(r / 23);
        state[4 * r + 2] = state[4 * r + 3] = 0.0f;
        ctrl[4 * r] = ctrl[4 * r + 1] = ctrl[4 * r + 2] = 0.0f;
        ctrl[4 * r + 3] = (float)(kRows - r);
    }
    const float lastX = state[4 * (kRows - 1)], lastY = state[4 * (kRows - 1) + 1];
    goals[0] = {1.0f, 1.0f, 0.625f};      // round row 0: rows 0, 1 and 23 inside
    goals[1] = {lastX, lastY, 0.25f};     // round the last row: it alone inside
    goals[2] = {6.0f, 6.0f, 1.25f};
    goals[3] = {lastX, 100.0f, 1.0f};     // nothing inside; the last row is the nearest
    goals[4] = {6.0f, 6.0f, -1.0f};       // a radius that admits nothing

    // a null mask and a mask of ones (any non-zero byte) give the same answers
    sbmp::query_rows_host(state, ctrl, nullptr, kRows, goals, kGoals, ref);
    if (ref[0].count != 3 || ref[0].firstRow != 0 || ref[0].bestRow != 23 || ref[0].nearestRow != 0)
        return fail("goal 0 over every row", ref[0].count, ref[0].bestRow);
    if (ref[1].count != 1 || ref[1].firstRow != kRows - 1 || ref[3].count != 0 || ref[3].nearestRow != kRows - 1)
        return fail("the last row", ref[1].firstRow, ref[3].nearestRow);
    if (ref[4].count != 0 || ref[4].bestRow != -1 || ref[4].nearestRow < 0) return fail("r = -1", ref[4].count, 0);
    const uint8_t bytes[5] = {1, 2, 0x7f, 0x80, 0xff};
    for (int r = 0; r < kRows; ++r) mask[r] = bytes[r % 5];
    sbmp::query_rows_host(state, ctrl, mask, kRows, goals, kGoals, out);
    for (int g = 0; g < kGoals; ++g)
        if (!same(out[g], ref[g])) return fail("a mask of non-zero bytes differs from no mask", g, out[g].count);

    // a mixed mask: rows 0 and 23 dead.  Goal 0 keeps row 1 alone, which is then first, best and nearest.
    mask[0] = mask[23] = 0;
    sbmp::query_rows_host(state, ctrl, mask, kRows, goals, kGoals, out);
    if (out[0].count != 1 || out[0].firstRow != 1 || out[0].bestRow != 1 || out[0].nearestRow != 1 ||
        out[0].bestCost != (float)(kRows - 1) || out[0].nearestDistance != 0.5f)
        return fail("goal 0 with rows 0 and 23 dead", out[0].count, out[0].nearestRow);
    for (int g = 1; g < kGoals; ++g)
        if (!same(out[g], ref[g])) return fail("a goal away from the dead rows changed", g, out[g].count);

    // the all-dead mask: the empty-set answer for every goal
    std::memset(mask, 0, kRows);
    sbmp::query_rows_host(state, ctrl, mask, kRows, goals, kGoals, out);
    for (int g = 0; g < kGoals; ++g)
        if (!empty(out[g])) return fail("the all-dead mask", g, out[g].nearestRow);

    // one alive row, at either end
    const int ends[2] = {0, kRows - 1};
    for (int e = 0; e < 2; ++e) {
        std::memset(mask, 0, kRows);
        mask[ends[e]] = 0x80;
        sbmp::query_rows_host(state, ctrl, mask, kRows, goals, kGoals, out);
        for (int g = 0; g < kGoals; ++g) {
            if (out[g].nearestRow != ends[e]) return fail("one alive row is not the nearest", g, out[g].nearestRow);
            const bool in = g == e;   // goal 0 holds row 0, goal 1 the last row
            if (out[g].count != (in ? 1 : 0) || out[g].firstRow != (in ? ends[e] : -1) || out[g].bestRow != out[g].firstRow)
                return fail("one alive row", g, out[g].count);
        }
    }
    delete[] state;
    delete[] ctrl;
    delete[] mask;

    // the one-row tree: alive, dead, unmasked
    float* s1 = new float[4];
    float* c1 = new float[4];
    uint8_t* m1 = new uint8_t[1];
    s1[0] = 6.25f, s1[1] = 6.0f, s1[2] = s1[3] = 0.0f;
    c1[0] = c1[1] = c1[2] = 0.0f, c1[3] = 7.0f;
    sbmp::query_rows_host(s1, c1, nullptr, 1, goals, kGoals, ref);
    if (ref[2].count != 1 || ref[2].bestRow != 0 || ref[2].bestCost != 7.0f || ref[2].nearestDistance != 0.25f)
        return fail("the one-row tree", ref[2].count, ref[2].bestRow);
    m1[0] = 1;
    sbmp::query_rows_host(s1, c1, m1, 1, goals, kGoals, out);
    for (int g = 0; g < kGoals; ++g)
        if (!same(out[g], ref[g])) return fail("the one-row tree, alive", g, out[g].count);
    m1[0] = 0;
    sbmp::query_rows_host(s1, c1, m1, 1, goals, kGoals, out);
    for (int g = 0; g < kGoals; ++g)
        if (!empty(out[g])) return fail("the one-row tree, dead", g, out[g].nearestRow);
    // count == 0 touches nothing
    sbmp::query_rows_host(s1, c1, m1, 1, nullptr, 0, nullptr);
    if (sbmp::goal_radius_threshold(0.5f) >= 0.25f || sbmp::goal_radius_threshold(-1.0f) != -1.0f)
        return fail("the threshold", 0, 0);
    delete[] s1;
    delete[] c1;
    delete[] m1;
    delete[] goals;
    delete[] out;
    delete[] ref;
    std::printf("ok\n");
    return 0;
}

// The host twin of the adoption rule (include/sbmp/tree_adopt.h) as a program of its own, over
// heap arrays of exactly the sizes the rule promises to stay inside: rows x 4 floats in, N * N
// ints per table and ceil(N * N * n * n / 32) bit words out.  tests/test_tree_adopt.py builds it
// with -fsanitize=address,undefined and runs it once: a write past a table, a read past the
// rows, or a float-to-int conversion out of range ends the program.  The rows stand on cell
// lines, outside the workspace on every side, at +-inf, NaN and the largest floats, over the
// smallest grid (N = n = 1), grids whose cells do not fill whole bit words and the largest one.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "sbmp/tree_adopt.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                                              \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            std::printf("%s:%d: %s (N %d, n %d, rows %d)\n", __FILE__, __LINE__, #cond, N, n, rows); \
            ++failures;                                                                           \
        }                                                                                         \
    } while (0)

void run(int N, int n, float width, int rows, int frontierFrom, bool withGoal) {
    std::unique_ptr<float[]> state(new float[4 * (size_t)rows]);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::numeric_limits<float>::max();
    const float R1Size = sbmp::adopt_r1_size(width, N), R2Size = sbmp::adopt_r2_size(width, N, n);
    const float special[] = {0.0f, -0.0f, -0.5f, -1.5f, width, std::nextafter(width, inf), std::nextafter(width, -inf),
                             inf, -inf, nan, big, -big, 3.0e9f, -3.0e9f, 2147483648.0f * R1Size};
    const int nSpecial = (int)(sizeof(special) / sizeof(special[0]));
    for (int r = 0; r < rows; ++r) {
        float x, y;
        if (r % 3 == 0) {   // on a line, or one ulp off it
            const float line = (float)(r % (N * n + 1)) * R2Size;
            x = (r % 9 == 0) ? line : (r % 9 == 3) ? std::nextafter(line, inf) : std::nextafter(line, -inf);
            y = (float)(r % (N + 1)) * R1Size;
        } else if (r % 3 == 1) {
            x = special[r % nSpecial];
            y = special[(r / nSpecial) % nSpecial];
        } else {
            x = width * (float)((r * 7919) % 1000) / 1000.0f;
            y = width * (float)((r * 104729) % 1000) / 1000.0f;
        }
        state[4 * (size_t)r + 0] = x;
        state[4 * (size_t)r + 1] = y;
        state[4 * (size_t)r + 2] = (r % 11 == 5) ? nan : 0.5f;
        state[4 * (size_t)r + 3] = (r % 13 == 7) ? -inf : 1.0f;
    }
    const int nR1 = N * N, nW = sbmp::adopt_r2_words(N, n);
    std::unique_ptr<int[]> R1(new int[nR1]), R1Avail(new int[nR1]), R1Valid(new int[nR1]), R1Invalid(new int[nR1]),
        R1Cov(new int[nR1]);
    std::unique_ptr<uint32_t[]> bits(new uint32_t[nW]);
    const float goal[3] = {width * 0.5f, width * 0.5f, width * 0.25f};
    sbmp_tree_adopt s;
    sbmp::adopt_tables_host(state.get(), rows, frontierFrom, width, N, n, withGoal ? goal : nullptr, R1.get(), R1Avail.get(),
                            R1Valid.get(), R1Invalid.get(), R1Cov.get(), bits.get(), &s);
    long long counted = 0, cov = 0, setBits = 0;
    for (int c = 0; c < nR1; ++c) {
        EXPECT(R1Valid[c] == R1[c]);
        EXPECT(R1Avail[c] == (R1[c] > 0 ? 1 : 0));
        EXPECT(R1Invalid[c] == 0);
        EXPECT(R1Cov[c] >= 0 && R1Cov[c] <= n * n);
        EXPECT((R1Cov[c] > 0) <= (R1[c] > 0));
        counted += R1[c];
        cov += R1Cov[c];
    }
    for (int w = 0; w < nW; ++w) setBits += __builtin_popcount(bits[w]);
    EXPECT(cov == setBits);
    EXPECT(counted <= rows && counted >= rows - s.outOfGrid);
    EXPECT(s.rows == rows && s.treeSize == rows && s.gLo == frontierFrom);
    EXPECT(s.frontierNonFinite <= s.nonFinite && s.nonFinite <= rows);
    EXPECT(s.goalRow >= -1 && s.goalRow < rows);
    EXPECT(withGoal || s.goalRow == -1);
    // every output may be null
    sbmp_tree_adopt s2;
    sbmp::adopt_tables_host(state.get(), rows, frontierFrom, width, N, n, withGoal ? goal : nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, &s2);
    EXPECT(std::memcmp(&s, &s2, sizeof(s)) == 0);
}

}  // namespace

int main() {
    const int grids[][2] = {{1, 1}, {1, 16}, {16, 1}, {3, 5}, {16, 8}, {16, 16}, {7, 3}};
    const float widths[] = {20.0f, 17.3f, 1.0e-3f, 4.0e6f};
    for (const auto& g : grids)
        for (float w : widths)
            for (int rows : {1, 2, 63, 257, 1500}) {
                run(g[0], g[1], w, rows, 0, false);
                run(g[0], g[1], w, rows, rows / 2, true);
                run(g[0], g[1], w, rows, rows, true);
            }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

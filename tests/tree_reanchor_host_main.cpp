// The host twin of the re-anchoring rule (include/sbmp/tree_reanchor.h) as a program of its own,
// over heap arrays of exactly the sizes the rule promises to stay inside: rows x 4 floats of
// state and controls and rows parents in, rows x 4 floats, rows alive bytes and rows status
// bytes out.  tests/test_tree_reanchor.py builds it with -fsanitize=address,undefined and runs it
// once: a read through an unusable parent, a read of a dead parent's state, or a write past the
// rows ends the program.  The trees are chains, stars and random parents, with crafted parents
// (-1, r, r + 1, INT_MIN, INT_MAX), car and point, with and without boxes, numDisc 1 and 10.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "sbmp/tree_reanchor.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                                                   \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            std::printf("%s:%d: %s (rows %d, shape %d, agent %d)\n", __FILE__, __LINE__, #cond, rows, shape, agent); \
            ++failures;                                                                                \
        }                                                                                              \
    } while (0)

unsigned lcg(unsigned& s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}
float uni(unsigned& s, float lo, float hi) { return lo + (hi - lo) * (float)(lcg(s) % 100000) / 100000.0f; }

// shape 0: a chain; 1: a star; 2: any lower row; 3: any lower row, and crafted parents
void run(int rows, int shape, int agent, int numDisc, int nObs) {
    std::unique_ptr<float[]> state(new float[4 * (size_t)rows]), ctrl(new float[4 * (size_t)rows]),
        out(new float[4 * (size_t)rows]);
    std::unique_ptr<int[]> parent(new int[(size_t)rows]);
    std::unique_ptr<uint8_t[]> alive(new uint8_t[(size_t)rows]), status(new uint8_t[(size_t)rows]);
    std::unique_ptr<float[]> boxes(new float[4 * (size_t)(nObs > 0 ? nObs : 1)]);
    unsigned seed = 12345u + (unsigned)rows * 7u + (unsigned)shape;
    for (int i = 0; i < nObs; ++i) {
        const float x = uni(seed, 0.0f, 18.0f), y = uni(seed, 0.0f, 18.0f);
        boxes[4 * i + 0] = x;
        boxes[4 * i + 1] = y;
        boxes[4 * i + 2] = x + 1.0f;
        boxes[4 * i + 3] = y + 1.0f;
    }
    const int crafted[] = {-1, 0, 1, INT_MIN, INT_MAX};   // 0: the row itself, 1: the next row
    for (int r = 0; r < rows; ++r) {
        for (int i = 0; i < 4; ++i) state[4 * (size_t)r + i] = uni(seed, 1.0f, 19.0f);
        ctrl[4 * (size_t)r + 0] = uni(seed, -5.0f, 5.0f);
        ctrl[4 * (size_t)r + 1] = uni(seed, -3.1f, 3.1f);
        ctrl[4 * (size_t)r + 2] = uni(seed, 0.06f, 0.4f);
        ctrl[4 * (size_t)r + 3] = 0.0f;
        int p = r == 0 ? -1 : shape == 0 ? r - 1 : shape == 1 ? 0 : (int)(lcg(seed) % (unsigned)r);
        if (shape == 3 && r > 0 && r % 7 == 3) {
            const int c = crafted[(r / 7) % 5];
            p = c == 0 ? r : c == 1 ? r + 1 : c;
        }
        parent[r] = p;
    }
    const float s0[4] = {10.0f, 10.0f, 0.3f, 0.5f};
    sbmp_tree_reanchor s;
    sbmp::reanchor_rows_host(state.get(), ctrl.get(), parent.get(), rows, s0, agent, numDisc, 1.0f, 20.0f, 20.0f,
                             nObs ? boxes.get() : nullptr, nObs, out.get(), alive.get(), status.get(), &s);
    EXPECT(s.rows == rows && s.rows == s.alive + s.blocked + s.orphan + s.cut);
    EXPECT(s.levels >= 1 && s.levels <= rows);
    EXPECT(shape != 0 || s.levels == rows);
    EXPECT(shape != 1 || s.levels == (rows > 1 ? 2 : 1));
    EXPECT(alive[0] == 1 && status[0] == SBMP_ROW_FREE && std::memcmp(out.get(), s0, sizeof(s0)) == 0);
    int firstDead = -1, nAlive = 0;
    for (int r = 0; r < rows; ++r) {
        const bool usable = sbmp::recheck_parent_usable(parent[r], r);
        nAlive += alive[r];
        EXPECT(alive[r] == (status[r] == SBMP_ROW_FREE ? 1 : 0));
        if (!alive[r] && firstDead < 0) firstDead = r;
        if (!alive[r]) EXPECT(std::memcmp(out.get() + 4 * (size_t)r, state.get() + 4 * (size_t)r, 4 * sizeof(float)) == 0);
        if (r > 0) EXPECT((status[r] == SBMP_ROW_ORPHAN) == !usable);
        if (r > 0 && usable) EXPECT((status[r] == (SBMP_ROW_FREE | SBMP_ROW_CUT)) == !alive[parent[r]]);
    }
    EXPECT(s.firstDead == firstDead && s.alive == nAlive);
    // status may be null
    sbmp_tree_reanchor s2;
    std::unique_ptr<float[]> out2(new float[4 * (size_t)rows]);
    sbmp::reanchor_rows_host(state.get(), ctrl.get(), parent.get(), rows, s0, agent, numDisc, 1.0f, 20.0f, 20.0f,
                             nObs ? boxes.get() : nullptr, nObs, out2.get(), alive.get(), nullptr, &s2);
    EXPECT(std::memcmp(&s, &s2, sizeof(s)) == 0);
    EXPECT(std::memcmp(out.get(), out2.get(), 4 * sizeof(float) * (size_t)rows) == 0);
}

}  // namespace

int main() {
    for (int rows : {1, 2, 3, 64, 257, 1500})
        for (int shape = 0; shape < 4; ++shape)
            for (int agent : {SBMP_AGENT_CAR, SBMP_AGENT_POINT})
                for (int numDisc : {1, 10})
                    for (int nObs : {0, 5}) run(rows, shape, agent, numDisc, nObs);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

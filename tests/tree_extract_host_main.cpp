// The host twin of the tree extraction (include/sbmp/tree_extract.h) as a program of its own,
// over heap arrays of exactly the sizes the rule promises to stay inside: rows x 4 floats, rows
// ints and rows bytes in, rows ints and kept rows out.  tests/test_tree_extract.py builds it with
// -fsanitize=address,undefined and runs it once: a read through a crafted parent word, or a
// write past the kept rows, ends the program.  Every crafted parent (-1, r, r + 1, INT_MIN,
// INT_MAX) stands on ordinary rows and on the root itself, with every row as the root.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "sbmp/tree_extract.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("%s:%d: %s (tree %s, root %d)\n", __FILE__, __LINE__, #cond, what, root); \
            ++failures;                                                                \
        }                                                                              \
    } while (0)

struct Tree {
    int rows;
    std::unique_ptr<float[]> state, ctrl;
    std::unique_ptr<int[]> parent;
    explicit Tree(int n) : rows(n), state(new float[4 * (size_t)n]), ctrl(new float[4 * (size_t)n]), parent(new int[n]) {
        for (int i = 0; i < 4 * n; ++i) {
            state[i] = 0.25f * (float)i;
            ctrl[i] = -1.5f * (float)i;
        }
    }
};

// Row r hangs on (r - 1) / 2: a binary heap.
Tree heap_tree(int n) {
    Tree t(n);
    for (int r = 0; r < n; ++r) t.parent[r] = r == 0 ? -1 : (r - 1) / 2;
    return t;
}

Tree chain_tree(int n) {
    Tree t(n);
    for (int r = 0; r < n; ++r) t.parent[r] = r - 1;
    return t;
}

void run(const Tree& t, int root, const uint8_t* keep, const char* what) {
    const int R = t.rows;
    std::unique_ptr<int[]> newRow(new int[R]);
    sbmp_tree_extract s;
    sbmp::extract_number_host(t.ctrl.get(), t.parent.get(), R, root, keep, newRow.get(), &s);
    EXPECT(s.rows == R && s.root == root);
    EXPECT(s.rows == s.kept + s.below + s.masked + s.detached);
    EXPECT(s.below == root);
    EXPECT(std::memcmp(&s.rootCost, &t.ctrl[4 * (size_t)root + 3], 4) == 0);
    const size_t k = (size_t)s.kept;
    // exactly `kept` rows each (new[0] is a valid, empty allocation)
    std::unique_ptr<float[]> oState(new float[4 * k]), oCtrl(new float[4 * k]);
    std::unique_ptr<int[]> oParent(new int[k]), oOrigin(new int[k]);
    sbmp::extract_gather_host(t.state.get(), t.ctrl.get(), t.parent.get(), R, root, newRow.get(), oState.get(),
                              oCtrl.get(), oParent.get(), oOrigin.get());
    int members = 0;
    for (int r = 0; r < R; ++r) {
        if (newRow[r] < 0) continue;
        EXPECT(newRow[r] == members);
        EXPECT(oOrigin[members] == r);
        EXPECT(!keep || keep[r] != 0);
        ++members;
    }
    EXPECT(members == s.kept);
    for (int i = 0; i < s.kept; ++i) {
        const int r = oOrigin[i];
        EXPECT(std::memcmp(&oState[4 * (size_t)i], &t.state[4 * (size_t)r], 16) == 0);
        EXPECT(std::memcmp(&oCtrl[4 * (size_t)i], &t.ctrl[4 * (size_t)r], 16) == 0);
        if (i == 0) {
            EXPECT(r == root && oParent[0] == -1);
        } else {
            EXPECT(oParent[i] >= 0 && oParent[i] < i && oOrigin[oParent[i]] == t.parent[r]);
        }
    }
    // the whole rule in one call gives the same, and an extraction extracts to itself
    std::unique_ptr<int[]> newRow2(new int[R]), again(new int[k ? k : 1]);
    std::unique_ptr<int[]> p2(new int[k]);
    sbmp_tree_extract s2;
    sbmp::extract_rows_host(t.state.get(), t.ctrl.get(), t.parent.get(), R, root, keep, newRow2.get(), nullptr, nullptr,
                            p2.get(), nullptr, &s2);
    EXPECT(std::memcmp(newRow.get(), newRow2.get(), sizeof(int) * (size_t)R) == 0);
    EXPECT(std::memcmp(&s, &s2, sizeof(s)) == 0);
    if (s.kept > 0) {
        sbmp_tree_extract s3;
        sbmp::extract_number_host(oCtrl.get(), oParent.get(), s.kept, 0, nullptr, again.get(), &s3);
        EXPECT(s3.kept == s.kept && s3.below == 0 && s3.masked == 0 && s3.detached == 0);
        for (int i = 0; i < s.kept; ++i) EXPECT(again[i] == i);
    }
}

void all_roots(Tree& t, const char* what) {
    const int R = t.rows;
    std::unique_ptr<uint8_t[]> alternating(new uint8_t[R]), odd(new uint8_t[R]);
    for (int r = 0; r < R; ++r) {
        alternating[r] = (uint8_t)(r % 2 == 0);
        odd[r] = (uint8_t)(r % 3 == 0 ? 0 : r % 3 == 1 ? 2 : 0x80);
    }
    for (int root = 0; root < R; ++root) {
        run(t, root, nullptr, what);
        run(t, root, alternating.get(), what);
        run(t, root, odd.get(), what);
    }
}

}  // namespace

int main() {
    const int crafted[5] = {-1, 0 /* r */, 1 /* r + 1 */, INT_MIN, INT_MAX};
    const int sizes[6] = {1, 2, 3, 64, 65, 257};
    for (int n : sizes) {
        Tree c = chain_tree(n);
        all_roots(c, "chain");
        Tree h = heap_tree(n);
        all_roots(h, "heap");
        for (int kind = 0; kind < 5; ++kind) {
            // on ordinary rows: 1, 5, the middle and the last; every one of them is a root in turn
            Tree t = heap_tree(n);
            const int at[4] = {1, 5, n / 2, n - 1};
            for (int r : at) {
                if (r < 0 || r >= n) continue;
                t.parent[r] = kind == 1 ? r : kind == 2 ? r + 1 : crafted[kind];
            }
            t.parent[0] = kind == 1 ? 0 : kind == 2 ? 1 : crafted[kind];   // and on row 0
            all_roots(t, "crafted");
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

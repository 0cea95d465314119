// The fold's rule (include/sbmp/r2_fold.h) as a stand-alone program, for a sanitizer build
// (tests/test_fold.py compiles it with -fsanitize=address,undefined and runs it once).  Ring, S,
// executed and both tables live in heap arrays sized to the byte, so a read one key past a row,
// one row past the ring, one entry past S or executed, or a write one cell past a table stops the
// program.  Checked against counts made the other way round (from the global slot to its owner
// rank and local index): windows that wrap the ring, with unexecuted iterations and stale
// in-grid keys at and past every S; three ranks whose folds must add up to the single-rank fold
// of the global log; the dropped keys.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "sbmp/r2_fold.h"

namespace {
constexpr int W = sbmp::kR2FoldWindow;

int fail(const char* what, int a, int b) {
    std::printf("FAILED: %s (%d, %d)\n", what, a, b);
    return 1;
}

uint32_t g_state = 0x2545f491u;
uint32_t next() {   // xorshift32
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return g_state;
}
uint16_t key_in(int nR2) { return (uint16_t)((next() % (uint32_t)nR2) | ((next() & 1u) << 15)); }

// The counts from the global slot's side: slot s of iteration t belongs to rank (s / 256) % P,
// local index ((s / 256) / P) * 256 + s % 256.
void expect(const uint16_t* const* rings, int P, int localSlots, const int* S, const int* ex, int tFirst, int T,
            int nR2, int onlyRank, long long* valid, long long* invalid) {
    for (int j = 0; j < T; ++j) {
        if (!ex[j]) continue;
        const int row = (tFirst + j) % W;
        const long long slots = (long long)P * localSlots;
        for (long long s = 0; s < slots && s < S[j]; ++s) {
            const int blk = (int)(s / 256), r = blk % P;
            if (onlyRank >= 0 && r != onlyRank) continue;
            const int i = (blk / P) * 256 + (int)(s % 256);
            const uint16_t k = rings[r][(size_t)row * localSlots + i];
            if (k == 0xffff || (k & 0x7fff) >= nR2) continue;
            ((k & 0x8000) ? valid : invalid)[k & 0x7fff] += 1;
        }
    }
}

int windows() {
    constexpr int L = 1024, nR2 = 2304;
    struct Win { int tFirst, T, holeFrom, holeTo; };
    const Win wins[] = {{0, 1, -1, -1}, {0, W, -1, -1}, {40, W, -1, -1}, {2 * W - 1, 1, -1, -1}, {31, W, 50, 57},
                        {5, W, 5, 5 + W - 1}};
    for (const Win& w : wins) {
        uint16_t* ring = new uint16_t[(size_t)W * L];
        int* S = new int[w.T];
        int* ex = new int[w.T];
        int* valid = new int[nR2];
        int* invalid = new int[nR2];
        long long* ev = new long long[nR2];
        long long* ei = new long long[nR2];
        for (size_t i = 0; i < (size_t)W * L; ++i) ring[i] = key_in(nR2);   // stale keys everywhere
        for (int j = 0; j < w.T; ++j) {
            const int t = w.tFirst + j;
            S[j] = (int)(8 * (next() % 120) + j % 8);
            if (j == 3) S[j] = L;
            if (j == 5) S[j] = 0;
            ex[j] = (t >= w.holeFrom && t <= w.holeTo) || (w.holeFrom == 50 && j == w.T - 1) ? 0 : 1;
            if (ex[j])
                for (int i = 0; i < S[j]; ++i) ring[(size_t)(t % W) * L + i] = (next() % 20 == 0) ? 0xffff : key_in(nR2);
        }
        for (int c = 0; c < nR2; ++c) valid[c] = 2, invalid[c] = 1, ev[c] = 2, ei[c] = 1;
        const uint16_t* rings[1] = {ring};
        expect(rings, 1, L, S, ex, w.tFirst, w.T, nR2, -1, ev, ei);
        sbmp::fold_r2_host(ring, S, ex, w.tFirst, w.tFirst + w.T - 1, L, nR2, 0, 1, valid, invalid);
        long long total = 0;
        for (int c = 0; c < nR2; ++c) {
            if (valid[c] != ev[c] || invalid[c] != ei[c]) return fail("window", w.tFirst, c);
            total += valid[c] + invalid[c] - 3;
        }
        if ((w.holeTo - w.holeFrom + 1 == W) != (total == 0)) return fail("window total", w.tFirst, (int)total);
        delete[] ring;
        delete[] S;
        delete[] ex;
        delete[] valid;
        delete[] invalid;
        delete[] ev;
        delete[] ei;
    }
    return 0;
}

int ranks() {
    constexpr int P = 3, blocks = 24, L = blocks / P * 256, nR2 = 2304;
    const int offs[6] = {0, 1, 7, 8, 9, 255};
    constexpr int T = 6 * P;
    uint16_t* ring[P];
    for (int r = 0; r < P; ++r) {
        ring[r] = new uint16_t[(size_t)W * L];
        for (size_t i = 0; i < (size_t)W * L; ++i) ring[r][i] = (next() % 20 == 0) ? 0xffff : key_in(nR2);
    }
    int* S = new int[T];
    int* ex = new int[T];
    for (int r = 0; r < P; ++r)
        for (int o = 0; o < 6; ++o) {
            S[6 * r + o] = (r + P * ((o + r) % (blocks / P))) * 256 + offs[o];
            ex[6 * r + o] = 1;
        }
    int* sumV = new int[nR2];
    int* sumI = new int[nR2];
    long long* allV = new long long[nR2];
    long long* allI = new long long[nR2];
    std::memset(sumV, 0, sizeof(int) * nR2);
    std::memset(sumI, 0, sizeof(int) * nR2);
    std::memset(allV, 0, sizeof(long long) * nR2);
    std::memset(allI, 0, sizeof(long long) * nR2);
    const uint16_t* rings[P] = {ring[0], ring[1], ring[2]};
    expect(rings, P, L, S, ex, 0, T, nR2, -1, allV, allI);
    for (int r = 0; r < P; ++r) {
        int* valid = new int[nR2];
        int* invalid = new int[nR2];
        long long* ev = new long long[nR2];
        long long* ei = new long long[nR2];
        for (int c = 0; c < nR2; ++c) valid[c] = invalid[c] = 0, ev[c] = ei[c] = 0;
        expect(rings, P, L, S, ex, 0, T, nR2, r, ev, ei);
        sbmp::fold_r2_host(ring[r], S, ex, 0, T - 1, L, nR2, r, P, valid, invalid);
        for (int c = 0; c < nR2; ++c)
            if (valid[c] != ev[c] || invalid[c] != ei[c]) return fail("rank", r, c);
        sbmp::fold_r2_host(ring[r], S, ex, 0, T - 1, L, nR2, r, P, sumV, sumI);   // all ranks into one pair
        delete[] valid;
        delete[] invalid;
        delete[] ev;
        delete[] ei;
    }
    for (int c = 0; c < nR2; ++c)
        if (sumV[c] != allV[c] || sumI[c] != allI[c]) return fail("the ranks' sum", c, sumV[c]);
    for (int r = 0; r < P; ++r) delete[] ring[r];
    delete[] S;
    delete[] ex;
    delete[] sumV;
    delete[] sumI;
    delete[] allV;
    delete[] allI;
    return 0;
}

int dropped() {
    constexpr int L = 256, nR2 = 1024;
    const uint16_t drop[] = {0xffff, 0x7fff, 1024, 1024 | 0x8000, 1025, 1025 | 0x8000, 1087, 1087 | 0x8000,
                             1088, 1088 | 0x8000, 0x7ffe, 0x7ffe | 0x8000};
    uint16_t* ring = new uint16_t[(size_t)W * L];
    int* valid = new int[nR2];
    int* invalid = new int[nR2];
    for (size_t i = 0; i < (size_t)W * L; ++i) ring[i] = drop[i % 12];
    ring[7] = 1023 | 0x8000;   // the last cell, in both kinds
    ring[8] = 1023;
    std::memset(valid, 0, sizeof(int) * nR2);
    std::memset(invalid, 0, sizeof(int) * nR2);
    const int S[1] = {L}, ex[1] = {1};
    sbmp::fold_r2_host(ring, S, ex, 0, 0, L, nR2, 0, 1, valid, invalid);
    for (int c = 0; c < nR2; ++c)
        if (valid[c] != (c == 1023) || invalid[c] != (c == 1023)) return fail("dropped keys", c, valid[c]);
    delete[] ring;
    delete[] valid;
    delete[] invalid;
    return 0;
}
}  // namespace

int main() {
    if (windows() || ranks() || dropped()) return 1;
    std::printf("ok\n");
    return 0;
}

// kgmt_rules.h — the reference's rules that more than one kernel applies, each stated
// once (D4, D6, D13, D18).  The kernels of kgmt_kernels.hip and the k_step
// body call these; csrc/batch.hip keeps its own statement on the public include/sbmp
// headers, as the audit tests' second hand.
// Every function is forced inline and takes what its callers hold in registers, and every
// kernel compiles to the instructions it had with the statements written out
// (tools/isa_diff.py against the parent build).  Four sites keep their statements because
// a call there changed a kernel's code: the k_step body's accept test (accept_test) and
// goal test (in_goal), plan_iteration's control block (make_ctrl), and updateR1's score
// and block sum (D17, D8), which both planners still write out.
#pragma once

#include "kgmt_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

// ------------------------------------------------------------------ insert (updateG)
// The updateG launch of an iteration that flagged A children: min(|GNew|, M/32) blocks of
// 32 threads (KGMT.cu:231), so only the first nIns = min(32 grid, A) flagged children
// become rows, and only GNew[0 .. 32 grid) is cleared (D6).
struct InsertLimits {
    int grid, nIns;
};
__device__ __forceinline__ InsertLimits insert_limits(int M, int A) {
    InsertLimits l;
    l.grid = min(A, M / 32);
    l.nIns = 32 * l.grid < A ? 32 * l.grid : A;
    return l;
}

// D6: the GNew bits [0, cleared) are cleared after the insert (KGMT.cu:231,556);
// fixGNewClear clears every bit.
__device__ __forceinline__ long long d6_cleared(int fixGNewClear, int grid) {
    return fixGNewClear ? (1ll << 62) : 32ll * grid;
}
// 64-bit GNew word `wordIndex` (bits 64 wordIndex ..) after that clear.
__device__ __forceinline__ unsigned long long d6_clear_word(unsigned long long word, int wordIndex, long long cleared) {
    const long long base = (long long)wordIndex * kWave;
    if (base + kWave <= cleared) return 0ull;
    if (base < cleared) return word & ~((1ull << (cleared - base)) - 1ull);
    return word;
}

// inGoalRegion (KGMT.cu:635-638, D18): pow(float, 2) is d * d in float, then sqrtf
// correctly rounded and < r (false for every r <= 0 and for NaN).
__device__ __forceinline__ bool in_goal(float x, float y, const KgmtDev& d) {
    const float dx = x - d.goalX, dy = y - d.goalY;
    const float d2 = dx * dx + dy * dy;
    return __builtin_sqrtf(d2) < d.goalThreshold;
}

// Tree row dst of the two-launch form (updateG, KGMT.cu:540-593), for a child the caller
// found inside the insert limits and below M (D13: the reference writes past M): cost =
// the parent's + the duration (getCost, KGMT.cu:631-633), plain stores, and the lowest row
// inside the goal radius is the solution (D4).
__device__ __forceinline__ void insert_row(const KgmtDev& d, int dst, const float4& state, const float4& ctrl) {
    const int parent = __float_as_int(ctrl.w);
    const float cost = d.treeCtrl[parent].w + ctrl.z;
    d.treeState[dst] = state;
    d.treeCtrl[dst] = make_float4(ctrl.x, ctrl.y, ctrl.z, cost);
    d.treeParent[dst] = parent;
    if (in_goal(state.x, state.y, d)) atomicMin(&d.status->goalIdx, dst);
}

// The same row in k_step: row tsPrev + j from a list entry, which carries the cost the
// expanding lane computed (the parent's + the duration, KGMT.cu:631-633) and whose goal
// test went into the block's packed count.  Written through (fewer dirty lines at the
// kernel boundary); the V# based at row tsPrev keeps the byte offset j * 16 far below 2^31
// whatever M is.
__device__ __forceinline__ void put_row(const KgmtDev& d, int tsPrev, int j, float4 s4, float4 u4, float cost) {
    store_wt(d.treeState + tsPrev, j, s4);
    store_wt(d.treeCtrl + tsPrev, j, make_float4(u4.x, u4.y, u4.z, cost));
    store_wt(d.treeParent + tsPrev, j, __float_as_int(u4.w));
}

// ------------------------------------------------------------------ regions (updateR1)
// A workgroup's R1 counters are packed (valid | invalid << 16) in LDS; its flush adds them
// to a 64-bit cell (valid | invalid << 32), whose replicas sum without carries.
__device__ __forceinline__ unsigned long long r1_delta_word(int v) {
    return (unsigned long long)(v & 0xffff) | ((unsigned long long)(v >> 16) << 32);
}
// That sum folded into one R1 cell's tables.
__device__ __forceinline__ void fold_r1_delta(unsigned long long dl, int& r1, int& r1v, int& r1i, int& r1a) {
    const int nv = (int)(dl & 0xffffffffull), ni = (int)(dl >> 32);
    r1 += nv + ni;      // every in-grid child (KGMT.cu:392)
    r1v += nv;          // KGMT.cu:406
    r1i += ni;          // KGMT.cu:409
    if (nv) r1a = 1;    // KGMT.cu:399-401
}
// One R2 key of the key log: r2 | valid << 15, kNoKey outside the R2 grid (D3).
__device__ __forceinline__ uint16_t r2_key(int q2, bool valid) {
    return (q2 >= 0) ? (uint16_t)(q2 | (valid ? 0x8000 : 0)) : kNoKey;
}

// KGMT.cu:527-535: an unavailable cell scores 1.
__device__ __forceinline__ float normalised_score(float sc, float total, int r1a) {
    return (r1a == 0) ? 1.0f : sc / total;
}

// R2New of 32 cells as one byte per cell (sums over ranks; <= nranks, so never a carry)
// -> one bit per cell: a nonzero byte is a cell seen valid while unavailable.
__device__ __forceinline__ uint32_t new_bits_from_bytes(uint4 b0, uint4 b1) {
    const uint32_t q[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    uint32_t nw = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // nonzero bytes -> 4 bits
        const uint32_t hi = (((q[k] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | q[k]) & 0x80808080u;
        nw |= ((((hi >> 7) * 0x00204081u) >> 21) & 0xfu) << (4 * k);
    }
    return nw;
}
// R1Cov (KGMT.cu:396-402): each R2 cell of word w that becomes available (`fresh`) counts
// once in its R1 cell, cell / n^2.  With n^2 a multiple of 32 the word lies in one R1 cell.
__device__ __forceinline__ void cov_add(int* sCovInc, uint32_t fresh, int w, int nn) {
    if (fresh && nn % 32 == 0) {
        atomicAdd(&sCovInc[(32 * w) / nn], __popc(fresh));
    } else {
        while (fresh) {
            const int k = __builtin_ctz(fresh);
            fresh &= fresh - 1u;
            atomicAdd(&sCovInc[(32 * w + k) / nn], 1);
        }
    }
}

// ------------------------------------------------------------------ plan and accept
// The control block of iteration t as its plan kernel writes it: A is filled in by the
// next plan kernel, the padding is zero.
__device__ __forceinline__ IterCtrl make_ctrl(int run, int executed, int treeSize, int gLo, int nG, int k, int nExp,
                                              int S, int H, int scoreBuf) {
    IterCtrl c;
    c.run = run;
    c.executed = executed;
    c.treeSize = treeSize;
    c.gLo = gLo;
    c.nG = nG;
    c.k = k;
    c.nExp = nExp;
    c.S = S;
    c.H = H;
    c.A = 0;
    c.scoreBuf = scoreBuf;
    for (int i = 0; i < 5; ++i) c.pad[i] = 0;
    return c;
}

// The accept test of a valid child in R2 cell q2 >= 0 (KGMT.cu:394-404) against the
// iteration-start snapshot (D2): u <= the score of its R1 cell, or its R2 cell was
// unavailable, which also sets the cell's R2New bit in the workgroup's LDS mask sNew.
// availWord is the snapshot word q2 >> 5.
__device__ __forceinline__ bool accept_test(float u, float score, uint32_t availWord, int q2, uint32_t* sNew) {
    const uint32_t bit = 1u << (q2 & 31);
    const bool r2Avail = availWord & bit;
    const bool accept = (u <= score) || !r2Avail;
    if (!r2Avail) atomicOr(&sNew[q2 >> 5], bit);
    return accept;
}

// Four waves each hold w_i flagged children and the index g_i (within the wave, kNoGoalIdx
// if none) of their first one in the goal region: the lowest wave holding one has the
// lowest index over all four (D4).
__device__ __forceinline__ int lowest_goal(int w0, int w1, int w2, int g0, int g1, int g2, int g3) {
    int jg = kNoGoalIdx;
    if (g3 != kNoGoalIdx) jg = w0 + w1 + w2 + g3;
    if (g2 != kNoGoalIdx) jg = w0 + w1 + g2;
    if (g1 != kNoGoalIdx) jg = w0 + g1;
    if (g0 != kNoGoalIdx) jg = g0;
    return jg;
}

// Diagnostics: where this wave runs, XCC id << 32 | HW_ID (wave, SIMD, CU, SE fields).
__device__ __forceinline__ long long placement_stamp() {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return ((long long)xcc << 32) | hw;
}

}  // namespace sbmp

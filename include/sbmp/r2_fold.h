// r2_fold.h — the fold of the R2 key log into R2Valid / R2Invalid, stated once as a plain
// host loop (the kernel is k_fold_r2, csrc/kgmt_kernels.hip).
//
// The expansion of iteration t logs one 16-bit key per child slot of this rank into row
// t % kR2FoldWindow of a ring [kR2FoldWindow][logSlots]:
//     key = cell | valid << 15      the child's R2 cell (< nR2 <= 32767) and its verdict
//     key = 0xffff                  the child lies outside the grid (D3)
// A row is written only below S(t), the slots iteration t expanded: at and past S(t) it
// still holds what iteration t - kR2FoldWindow, or an earlier plan, left there.
//
// The fold of iterations [tFirst, tLast], at most kR2FoldWindow of them, is, for every t
// with executed[t] != 0 and every local key index i < logSlots:
//     slot = (rank + nranks * (i / 256)) * 256 + i % 256      the global slot of local key i
//            (256-slot blocks are dealt to the ranks round-robin; one rank: slot = i)
//     key  = ring[(t % kR2FoldWindow) * logSlots + i]
//     the key counts  iff  slot < S[t]  and  (key & 0x7fff) < nR2
//     a counting key adds 1 to R2Valid[key & 0x7fff] when bit 15 is set, else to
//     R2Invalid[key & 0x7fff]
// The tables are in/out: the counts are added to what they hold.  0xffff, 0x7fff and every
// other cell >= nR2 count nowhere (the planner writes only 0xffff; the kernel sends all of
// them to sink words past its histogram).  An iteration that did not execute adds nothing,
// whatever its row and its S hold.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sbmp {

constexpr int kR2FoldWindow = 64;     // rows of the key ring = iterations per fold
constexpr int kR2KeyCellMask = 0x7fff;
constexpr int kR2KeyValidBit = 0x8000;
constexpr int kR2FoldBlock = 256;     // slots per block, the unit dealt to ranks

// S and executed hold one entry per iteration, entry j for iteration tFirst + j.
inline void fold_r2_host(const uint16_t* ring, const int* S, const int* executed, int tFirst, int tLast,
                         int logSlots, int nR2, int rank, int nranks, int* R2Valid, int* R2Invalid) {
    for (int t = tFirst; t <= tLast; ++t) {
        if (!executed[t - tFirst]) continue;
        const uint16_t* row = ring + (size_t)(t % kR2FoldWindow) * (size_t)logSlots;
        const long long s = S[t - tFirst];
        for (int i = 0; i < logSlots; ++i) {
            const long long slot = ((long long)rank + (long long)nranks * (i / kR2FoldBlock)) * kR2FoldBlock +
                                   i % kR2FoldBlock;
            if (slot >= s) continue;
            const int key = row[i];
            const int cell = key & kR2KeyCellMask;
            if (cell >= nR2) continue;
            if (key & kR2KeyValidBit) R2Valid[cell] += 1;
            else R2Invalid[cell] += 1;
        }
    }
}

}  // namespace sbmp

// fold_batch.cpp — the step-level entry of the R2 key-log fold (include/sbmp/sbmp.h):
//   sbmp_fold_r2_batch        k_fold_r2 over a caller ring, through launch_fold_r2 (the planner's
//                             own split into workgroups and LDS opt-in)
//   sbmp_fold_r2_batch_host   the rule's host loop (include/sbmp/r2_fold.h)
//   sbmp_fold_r2_info         the constants and the launcher's split
// No kernel lives here: the entry fills the KgmtDev fields k_fold_r2 reads (r2log, logSlots,
// nR2, rank, nranks, ctrl, R2Valid, R2Invalid) and nothing else.
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/r2_fold.h"
#include "sbmp/sbmp.h"

namespace sbmp {

static_assert(kFoldEvery == kR2FoldWindow, "the rule header and the kernel share the window");
static_assert(kBlock == kR2FoldBlock, "the rule header and the kernel share the block size");
static_assert(kNoKey == 0xffff && kLogMaxR2 == kR2KeyCellMask, "the key layout of the rule header");

// the device entry holds one 64-B control block per iteration up to tLast, as the planner does
constexpr int kFoldMaxIteration = 1 << 20;

static void check_fold(const void* ring, const int* S, const int* executed, int tFirst, int tLast, int logSlots,
                       int nR2, int rank, int nranks, const int* valid, const int* invalid) {
    if (!ring || !S || !executed || !valid || !invalid) throw Error(SBMP_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (logSlots <= 0 || logSlots % kBlock != 0)
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "logSlots must be a positive multiple of 256");
    if (nR2 < 1 || nR2 > kLogMaxR2) throw Error(SBMP_ERR_INVALID_ARGUMENT, "nR2 outside [1, 32767]");
    if (tFirst < 0) throw Error(SBMP_ERR_INVALID_ARGUMENT, "tFirst < 0");
    // (in 64 bits: tLast - tFirst may not fit an int)
    const long long T = (long long)tLast - (long long)tFirst + 1;
    if (T < 1 || T > kFoldEvery) throw Error(SBMP_ERR_INVALID_ARGUMENT, "tLast - tFirst + 1 outside [1, 64]");
    if (tLast >= kFoldMaxIteration) throw Error(SBMP_ERR_INVALID_ARGUMENT, "tLast >= 2^20");
    if (nranks < 1 || nranks > kMaxRanks) throw Error(SBMP_ERR_INVALID_ARGUMENT, "nranks outside [1, 8]");
    if (rank < 0 || rank >= nranks) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rank outside [0, nranks)");
}

void fold_r2_info(int logSlots, sbmp_fold_info* out) {
    if (!out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "NULL out");
    if (logSlots <= 0 || logSlots % kBlock != 0)
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "logSlots must be a positive multiple of 256");
    out->window = kFoldEvery;
    out->keysPerGroup = kFoldKeys;
    out->maxR2 = kLogMaxR2;
    out->maxRanks = kMaxRanks;
    fold_split(logSlots, &out->groups, &out->per);
}

void fold_r2_batch_host(const uint16_t* ring, const int* S, const int* executed, int tFirst, int tLast, int logSlots,
                        int nR2, int rank, int nranks, int* valid, int* invalid) {
    check_fold(ring, S, executed, tFirst, tLast, logSlots, nR2, rank, nranks, valid, invalid);
    fold_r2_host(ring, S, executed, tFirst, tLast, logSlots, nR2, rank, nranks, valid, invalid);
}

void fold_r2_batch(const uint16_t* d_ring, const int* S, const int* executed, int tFirst, int tLast, int logSlots,
                   int nR2, int rank, int nranks, int* d_valid, int* d_invalid, hipStream_t s) {
    check_fold(d_ring, S, executed, tFirst, tLast, logSlots, nR2, rank, nranks, d_valid, d_invalid);
    // the kernel reads ctrl[t] by the iteration's own number: entries below tFirst stay zero
    std::vector<IterCtrl> ctrl((size_t)tLast + 1, IterCtrl{});
    for (int t = tFirst; t <= tLast; ++t) {
        ctrl[t].executed = executed[t - tFirst] ? 1 : 0;
        ctrl[t].S = S[t - tFirst] > 0 ? S[t - tFirst] : 0;   // no slot lies below an S <= 0
    }
    KgmtDev d{};
    d.r2log = const_cast<uint16_t*>(d_ring);
    d.logSlots = logSlots;
    d.nR2 = nR2;
    d.rank = rank;
    d.nranks = nranks;
    d.R2Valid = d_valid;
    d.R2Invalid = d_invalid;
    SBMP_HIP(hipMalloc(reinterpret_cast<void**>(&d.ctrl), sizeof(IterCtrl) * ctrl.size()));
    hipError_t e = hipMemcpyAsync(d.ctrl, ctrl.data(), sizeof(IterCtrl) * ctrl.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // ctrl is pageable host memory that ends with this call
    if (e == hipSuccess) {
        (void)hipGetLastError();
        launch_fold_r2(d, tFirst, tLast, s);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(d.ctrl);
    SBMP_HIP(e);
    SBMP_HIP(e2);
}

}  // namespace sbmp

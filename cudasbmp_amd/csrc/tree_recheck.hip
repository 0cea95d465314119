// tree_recheck.hip — a grown tree re-checked against another obstacle list
// (include/sbmp/tree_recheck.h states the rule).
//   k_tree_recheck<AGENT, OBS>  one lane per row: the row's parent first; behind the orphan
//                               test the parent's state, the row's controls and state; then the
//                               expand step's own Euler loop (car_euler / point_euler) against the
//                               new list, and one status byte
//   k_tree_alive<LAST>          alive[r] = FREE along the whole parent chain, by pointer jumping
//                               over double-buffered (anc, dead) arrays: dead'[r] = dead[r] |
//                               dead[anc[r]], anc'[r] = anc[anc[r]].  The status bytes are the
//                               first dead array (FREE is 0).  The last pass writes the exported
//                               bytes, the alive mask and the summary.
//   sbmp_tree_recheck_batch / _host, sbmp_kgmt_recheck_tree
// The goal query over the alive mask (k_tree_query_alive) lives in tree_query.hip, beside the
// query it masks; the grids, the buffers and the read-back are tree_pass.h's.
// No workgroup waits for another inside a kernel: stream order between the launches is the
// only ordering.  Every pass reads one buffer pair and writes the other, and the summary is
// integer adds and one unsigned minimum, so the bytes and the counts do not depend on the
// grid or on the order rows arrive in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "obstacle_grid.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_recheck.h"
#include "tree_pass.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

namespace {
constexpr int kRecheckBlock = 256;   // lanes per workgroup, one row per lane and sweep
// Workgroups per CU the grids are sized for, at most (the occupancy query may give fewer):
// one sweep is at most CUs x 8 x 256 rows, longer trees go round the grid-stride loops again.
constexpr int kRecheckGroupsPerCU = 8;

// The summary's accumulators (device): integer adds and one unsigned minimum.
struct RecheckAcc {
    unsigned alive, blocked, stale, orphan, cut;
    unsigned firstDead;   // ~0u: none
};

// (anc0, status): the first buffer pair of k_tree_alive.  A row that is not FREE, and the root,
// point at themselves: nothing is ever loaded through an orphan's parent word.
template <int AGENT, int OBS>
__global__ __launch_bounds__(kRecheckBlock) void k_tree_recheck(KgmtDev d, unsigned rows, uint8_t* __restrict__ status,
                                                                int* __restrict__ anc0) {
    extern __shared__ float4 sObs[];
    constexpr bool kLdsObs = (OBS == kObsLds || OBS == kObsLds4);
    constexpr int kRegObs = obs_in_registers(OBS);
    float4 ro[kRegObs > 0 ? kRegObs : 1];   // register-resident obstacle list
#pragma unroll
    for (int i = 0; i < kRegObs; ++i) {
        ro[i] = d.obstacles[i];
        // The list in vector registers: as uniform values the compiler keeps the 4 n floats in
        // SGPRs next to the plan's parameters and the row loop's state, and ran out of them
        // from three boxes on (SGPRs spilled to VGPR lanes).  VGPRs are plentiful here.
        asm volatile("" : "+v"(ro[i].x), "+v"(ro[i].y), "+v"(ro[i].z), "+v"(ro[i].w));
    }
    if (kLdsObs) {
        for (int i = threadIdx.x; i < d.nObs; i += kRecheckBlock) sObs[i] = d.obstacles[i];
        __syncthreads();
    }
    const float4* obs = (kRegObs > 0) ? ro : kLdsObs ? sObs : d.obstacles;
    // The row loop's five pointers in vector registers, for the same reason: the car's LDS-4 and
    // grid forms were a few SGPRs short across the Euler loop.
    const float4* tState = d.treeState;
    const float4* tCtrl = d.treeCtrl;
    const int* tParent = d.treeParent;
    asm volatile("" : "+v"(status), "+v"(anc0), "+v"(tState), "+v"(tCtrl), "+v"(tParent));

    // unsigned: rows < 2^31 and a sweep is at most 2^19 rows, so row + stride cannot wrap
    const unsigned stride = gridDim.x * kRecheckBlock;
    for (unsigned row = blockIdx.x * kRecheckBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const int parent = tParent[r];
        uint8_t st = SBMP_ROW_FREE;
        if (r > 0) {
            if (!recheck_parent_usable(parent, r)) {
                st = SBMP_ROW_ORPHAN;
            } else {
                const float4 p = tState[parent];
                const float4 c = tCtrl[r];
                const float4 me = tState[r];
                const ChildCtl ctl = stored_controls<AGENT>(c, d);
                ChildOut out;
                const bool valid = (AGENT == 0) ? car_euler<OBS>(p, ctl, d, obs, out) : point_euler<OBS>(p, ctl, d, obs, out);
                st = recheck_replayed_status(valid, recheck_same_state(out.state.x, out.state.y, out.state.z,
                                                                       out.state.w, me.x, me.y, me.z, me.w));
            }
        }
        status[r] = st;
        anc0[r] = (st == SBMP_ROW_FREE && r > 0) ? parent : r;
    }
}

// One pointer-jumping pass: deadIn[r] != 0 iff some row of r's chain covered so far is not FREE.
// LAST: the pass that turns that into the exported bytes (deadOut), the alive mask (alive may be
// null) and the summary; it writes no anc.  status: k_tree_recheck's bytes (LAST only; it may be
// deadIn as well, both are only read).
template <bool LAST>
__global__ __launch_bounds__(kRecheckBlock) void k_tree_alive(const int* __restrict__ ancIn, const uint8_t* deadIn,
                                                              int* __restrict__ ancOut, uint8_t* __restrict__ deadOut,
                                                              int rows, const uint8_t* status,
                                                              uint8_t* __restrict__ alive, RecheckAcc* __restrict__ acc) {
    __shared__ unsigned sAcc[6];
    if (LAST) {
        if (threadIdx.x < 6) sAcc[threadIdx.x] = threadIdx.x == 5 ? ~0u : 0u;
        __syncthreads();
    }
    unsigned nAlive = 0, nBlocked = 0, nStale = 0, nOrphan = 0, nCut = 0, first = ~0u;
    const long long stride = (long long)gridDim.x * kRecheckBlock;
    for (long long row = (long long)blockIdx.x * kRecheckBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const int a = ancIn[r];   // a row of [0, r], by construction (k_tree_recheck, and jumps only go up)
        const uint8_t dead = deadIn[r] | deadIn[a];
        if (!LAST) {
            deadOut[r] = dead;
            ancOut[r] = ancIn[a];
        } else {
            const uint8_t e = recheck_export_byte(status[r], dead == 0);
            deadOut[r] = e;
            if (alive) alive[r] = dead == 0 ? 1 : 0;
            nAlive += e == SBMP_ROW_FREE;
            nBlocked += e == SBMP_ROW_BLOCKED;
            nStale += e == SBMP_ROW_STALE;
            nOrphan += e == SBMP_ROW_ORPHAN;
            nCut += e == (SBMP_ROW_FREE | SBMP_ROW_CUT);
            if (e != SBMP_ROW_FREE && (unsigned)r < first) first = (unsigned)r;
        }
    }
    if (LAST) {
        if (nAlive) atomicAdd(&sAcc[0], nAlive);
        if (nBlocked) atomicAdd(&sAcc[1], nBlocked);
        if (nStale) atomicAdd(&sAcc[2], nStale);
        if (nOrphan) atomicAdd(&sAcc[3], nOrphan);
        if (nCut) atomicAdd(&sAcc[4], nCut);
        if (first != ~0u) atomicMin(&sAcc[5], first);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (sAcc[0]) atomicAdd(&acc->alive, sAcc[0]);
            if (sAcc[1]) atomicAdd(&acc->blocked, sAcc[1]);
            if (sAcc[2]) atomicAdd(&acc->stale, sAcc[2]);
            if (sAcc[3]) atomicAdd(&acc->orphan, sAcc[3]);
            if (sAcc[4]) atomicAdd(&acc->cut, sAcc[4]);
            if (sAcc[5] != ~0u) atomicMin(&acc->firstDead, sAcc[5]);
        }
    }
}

// ---------------------------------------------------------------- host side
// Workgroups of kRecheckBlock lanes for `rows` rows (resident_grid, tree_pass.h).
template <class Kernel>
int recheck_grid(Kernel* fn, size_t lds, long long rows, const char* name) {
    return resident_grid(fn, kRecheckBlock, lds, kRecheckGroupsPerCU, rows, name);
}

using RecheckFn = decltype(&k_tree_recheck<0, kObsGlobal>);

// Per-call scratch (in w): the status bytes, two anc and two dead arrays (twoPairs; else only
// anc[0] and dead[1] are used) and the accumulators.
struct RecheckScratch {
    uint8_t* status;
    int* anc[2] = {nullptr, nullptr};
    uint8_t* dead[2] = {nullptr, nullptr};
    RecheckAcc* acc;
    RecheckScratch(DevBufs& w, size_t rows, bool twoPairs) {
        status = w.alloc<uint8_t>(rows);
        for (int i = 0; i < 2; ++i) {
            if (i == 0 || twoPairs) anc[i] = w.alloc<int>(rows);
            if (i == 1 || twoPairs) dead[i] = w.alloc<uint8_t>(rows);
        }
        acc = w.alloc<RecheckAcc>(1);
    }
};

// ceil(log2(bound)): after that many passes dead[r] covers 2^passes >= bound rows of r's chain.
int jump_passes(long long bound) {
    int p = 0;
    while ((1ll << p) < bound) ++p;
    return p;
}

}  // namespace

void tree_recheck_device(const KgmtDev& base, int agent, int variant, int rows, int depthBound,
                         const float* d_obstacles, int nObs, uint8_t* d_alive, uint8_t* status,
                         sbmp_tree_recheck* out, hipStream_t stream) {
    if (rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    if (nObs < 0 || (nObs > 0 && !d_obstacles)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad obstacle list");
    if (!out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "out must be non-NULL");
    KgmtDev d = base;   // the plan's own struct, list and grid stay untouched
    DevBufs listBufs, scratchBufs;   // freed with the call: the scratch first, then the list
    RecheckAcc acc;
    drained_on_throw(stream, [&] {
        attach_list(listBufs, d, d_obstacles, nObs, variant, stream);
        const int passes = std::max(1, jump_passes(depthBound > 0 ? std::min(depthBound, rows) : rows));
        const RecheckScratch w(scratchBufs, (size_t)rows, passes > 1);
        SBMP_HIP(hipMemsetAsync(w.acc, 0, sizeof(RecheckAcc), stream));
        SBMP_HIP(hipMemsetAsync(&w.acc->firstDead, 0xff, sizeof(unsigned), stream));
        with_obs_form(d, variant, [&](auto obs) {
            const RecheckFn fn = (agent == SBMP_AGENT_POINT) ? k_tree_recheck<1, obs.value> : k_tree_recheck<0, obs.value>;
            const size_t lds = (obs.value == kObsLds || obs.value == kObsLds4) ? sizeof(float4) * (size_t)d.nObs : 0;
            const int grid = recheck_grid(fn, lds, rows, "k_tree_recheck");
            hipLaunchKernelGGL(fn, dim3(grid), dim3(kRecheckBlock), lds, stream, d, (unsigned)rows, w.status, w.anc[0]);
        });
        // pass p reads (anc[p & 1], dead of p) and writes (anc[(p + 1) & 1], dead[(p + 1) & 1]);
        // the dead array of pass 0 is the status bytes themselves
        auto deadIn = [&](int p) { return p == 0 ? w.status : w.dead[p & 1]; };
        const int gridA = recheck_grid(k_tree_alive<false>, 0, rows, "k_tree_alive");
        for (int p = 0; p + 1 < passes; ++p)
            hipLaunchKernelGGL(k_tree_alive<false>, dim3(gridA), dim3(kRecheckBlock), 0, stream, w.anc[p & 1],
                               (const uint8_t*)deadIn(p), w.anc[(p + 1) & 1], w.dead[(p + 1) & 1], rows,
                               (const uint8_t*)nullptr, (uint8_t*)nullptr, (RecheckAcc*)nullptr);
        const int last = passes - 1;
        uint8_t* const exported = w.dead[(last + 1) & 1];
        hipLaunchKernelGGL(k_tree_alive<true>, dim3(gridA), dim3(kRecheckBlock), 0, stream, w.anc[last & 1],
                           (const uint8_t*)deadIn(last), (int*)nullptr, exported, rows, (const uint8_t*)w.status, d_alive,
                           w.acc);
        SBMP_HIP(hipGetLastError());
        read_back(stream, {{&acc, w.acc, sizeof(acc)}, {status, exported, (size_t)rows}});
    });
    out->rows = rows;
    out->alive = (int)acc.alive;
    out->blocked = (int)acc.blocked;
    out->stale = (int)acc.stale;
    out->orphan = (int)acc.orphan;
    out->cut = (int)acc.cut;
    out->firstDead = acc.firstDead == ~0u ? -1 : (int)acc.firstDead;
}

namespace {
void check_recheck_args(const sbmp_tree_recheck_args* a, const sbmp_tree_recheck* out) {
    if (!a || !out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "args and out must be non-NULL");
    if (!a->state || !a->ctrl || !a->parent) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and parent must be non-NULL");
    if (a->rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    if (a->numDisc < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "numDisc must be >= 1");
    if (a->obstaclesCount < 0 || (a->obstaclesCount > 0 && !a->obstacles))
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad obstacle list");
    if (a->agent != SBMP_AGENT_CAR && a->agent != SBMP_AGENT_POINT) throw Error(SBMP_ERR_INVALID_ARGUMENT, "agent");
}
}  // namespace

void tree_recheck_batch(const sbmp_tree_recheck_args* a, uint8_t* status, sbmp_tree_recheck* out, hipStream_t stream) {
    check_recheck_args(a, out);
    KgmtDev d{};
    set_euler_params(d, a->numDisc, a->agentLength);
    d.width = a->width;
    d.height = a->height;
    d.treeState = reinterpret_cast<float4*>(const_cast<float*>(a->state));
    d.treeCtrl = reinterpret_cast<float4*>(const_cast<float*>(a->ctrl));
    d.treeParent = const_cast<int*>(a->parent);
    const int variant = expand_variant_from_env();
    tree_recheck_device(d, a->agent, variant, a->rows, a->depthBound, a->obstacles, a->obstaclesCount, nullptr, status,
                        out, stream);
}

void tree_recheck_batch_host(const sbmp_tree_recheck_args* a, uint8_t* status, sbmp_tree_recheck* out) {
    check_recheck_args(a, out);
    std::vector<uint8_t> alive((size_t)a->rows);
    recheck_rows_host(a->state, a->ctrl, a->parent, a->rows, a->agent, a->numDisc, a->agentLength, a->width, a->height,
                      a->obstacles, a->obstaclesCount, alive.data(), status, out);
}

}  // namespace sbmp

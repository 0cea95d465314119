// tree_reanchor.hip — a grown tree re-anchored on a measured root state, level by level
// (include/sbmp/tree_reanchor.h states the rule).
//   k_reanchor_init       one lane per row: anc = the parent if usable, else the row; hop = 1 / 0
//   k_reanchor_jump       one pointer-jumping pass over double buffers: hop'[r] = hop[r] +
//                         hop[anc[r]], anc'[r] = anc[anc[r]].  After p passes hop[r] is the row's
//                         edges to the top of its chain (row 0 or an orphan), if those are <= 2^p
//   k_reanchor_hist       the rows of every depth (one add per distinct depth of a wave, into an LDS
//                         histogram where the depths fit), and the flag of a short bound: a row
//                         whose anc is not yet a top
//   k_reanchor_offsets    one workgroup: the exclusive sum of the depth counts (the level
//                         offsets, and the cursors of the scatter) and `levels`
//   k_reanchor_scatter    order[]: the rows of level 0, then of level 1, ...; one atomic per
//                         distinct depth of a wave.  The order inside a level is arbitrary
//   k_reanchor_level<AGENT, OBS>  one launch per level over its slice of order[]: the parent's
//                         alive byte, then its NEW state and the row's controls through the expand
//                         step's own Euler loop (car_euler / point_euler); status, alive, out[r]
//   sbmp_tree_reanchor_batch / _host, and what KgmtPlanner::reanchor_tree / replan_from run
// The replay of a row reads what the launch of its parent's level wrote: stream order between
// the launches is the only ordering, and no workgroup waits for another.  Every row is written
// by exactly one lane from values that do not depend on where it stands in order[], and the
// summary is integer adds and one unsigned minimum, so no output byte depends on the grid or on
// the order the atomics hand out.  Row indices are 32-bit; every byte offset (16 x row) is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_reanchor.h"
#include "tree_pass.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

namespace {
constexpr int kReanchorBlock = 256;        // lanes per workgroup
constexpr int kReanchorWaves = kReanchorBlock / 64;
constexpr int kReanchorGroupsPerCU = 8;    // as the re-check's passes
constexpr int kReanchorLdsDepths = 2048;   // depth counters a workgroup privatises in LDS (8 KB)

// The summary's accumulators (device): integer adds and one unsigned minimum.
struct ReanchorAcc {
    unsigned alive, blocked, orphan, cut;
    unsigned firstDead;   // ~0u: none
};

// What the host reads before the levels, one copy: meta[0] the short-bound flag, meta[1] levels,
// then the level offsets off[0 .. depths] (off[depths] = rows).
constexpr int kReanchorMeta = 2;

__global__ __launch_bounds__(kReanchorBlock) void k_reanchor_init(const int* __restrict__ parent, int rows,
                                                                  int* __restrict__ anc0, int* __restrict__ hop0) {
    const long long stride = (long long)gridDim.x * kReanchorBlock;
    for (long long row = (long long)blockIdx.x * kReanchorBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const int p = parent[r];
        const bool usable = recheck_parent_usable(p, r);   // never for row 0
        anc0[r] = usable ? p : r;
        hop0[r] = usable ? 1 : 0;
    }
}

// ancIn[r] is a row of [0, r] by construction (k_reanchor_init, and jumps only go up); a top
// points at itself with hop 0, so a chain that has arrived stays as it is.
__global__ __launch_bounds__(kReanchorBlock) void k_reanchor_jump(const int* __restrict__ ancIn,
                                                                  const int* __restrict__ hopIn,
                                                                  int* __restrict__ ancOut, int* __restrict__ hopOut,
                                                                  int rows) {
    const long long stride = (long long)gridDim.x * kReanchorBlock;
    for (long long row = (long long)blockIdx.x * kReanchorBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const int a = ancIn[r];
        hopOut[r] = hopIn[r] + hopIn[a];
        ancOut[r] = ancIn[a];
    }
}

// count[h] += the rows of depth h.  hop[r] <= r and hop[r] <= 2^passes, so hop[r] < depths, the
// counters the host allocated (min(rows, 2^passes + 1)), whatever the bound was.  A row whose anc
// is not a fixed point has not reached its top: the bound was too short, and its hop is no depth.
__global__ __launch_bounds__(kReanchorBlock) void k_reanchor_hist(const int* __restrict__ anc,
                                                                  const int* __restrict__ hop, int rows, int depths,
                                                                  int* __restrict__ count, int* __restrict__ meta) {
    __shared__ int sHist[kReanchorLdsDepths];
    const bool inLds = depths <= kReanchorLdsDepths;   // uniform
    if (inLds) {
        for (int i = threadIdx.x; i < depths; i += kReanchorBlock) sHist[i] = 0;
        __syncthreads();
    }
    bool shortBound = false;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kReanchorBlock;
    for (long long base = (long long)blockIdx.x * kReanchorBlock; base < rows; base += stride) {   // uniform
        const long long row = base + threadIdx.x;
        const bool in = row < rows;
        int h = -1;
        if (in) {
            const int a = anc[row];
            shortBound |= anc[a] != a;
            h = hop[row];
        }
        // one add per distinct depth of a wave, by the lowest lane that holds it: a star's 2^20 rows
        // of one depth are 2^14 adds on its counter, not 2^20 (with one add a row the call took
        // 15.7 ms instead of 4.3 where the depths do not fit in LDS: depthBound 0)
        unsigned long long todo = __ballot(in);
        while (todo) {   // uniform
            const int leader = (int)__builtin_ctzll(todo);
            const int v = __builtin_amdgcn_readlane(h, leader);
            const unsigned long long same = __ballot(h == v);
            if (lane == leader) {
                if (inLds) atomicAdd(&sHist[v], (int)__popcll(same));
                else atomicAdd(&count[v], (int)__popcll(same));
            }
            todo &= ~same;
        }
    }
    if (shortBound) atomicOr(&meta[0], 1);
    if (inLds) {
        __syncthreads();
        for (int i = threadIdx.x; i < depths; i += kReanchorBlock)
            if (sHist[i]) atomicAdd(&count[i], sHist[i]);
    }
}

// One workgroup: off[h] = cursor[h] = the rows of the depths before h, off[depths] = all rows,
// meta[1] = 1 + the deepest depth that has a row.  A round takes kReanchorBlock depths, one per
// lane; `base` carries the rounds before in a register.
__global__ __launch_bounds__(kReanchorBlock) void k_reanchor_offsets(const int* __restrict__ count, int depths,
                                                                     int* __restrict__ off, int* __restrict__ cursor,
                                                                     int* __restrict__ meta) {
    __shared__ int sWave[kReanchorWaves];
    __shared__ int sLevels;
    if (threadIdx.x == 0) sLevels = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0, levels = 0;
    for (int h0 = 0; h0 < depths; h0 += kReanchorBlock) {   // uniform: every lane is active in wave_incl_sum
        const int h = h0 + (int)threadIdx.x;
        const int c = h < depths ? count[h] : 0;
        if (c > 0) levels = h + 1;
        const int incl = wave_incl_sum(c);
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kReanchorWaves; ++i) {
            const int v = sWave[i];
            before += i < wave ? v : 0;
            total += v;
        }
        if (h < depths) {
            off[h] = base + before + incl - c;
            cursor[h] = base + before + incl - c;
        }
        base += total;
        __syncthreads();   // sWave is written again in the next round
    }
    if (levels) atomicMax(&sLevels, levels);
    __syncthreads();
    if (threadIdx.x == 0) {
        off[depths] = base;
        meta[1] = sLevels;
    }
}

// order[cursor[hop[r]]++] = r.  One atomic per distinct depth of a wave, by the lowest lane that
// holds it; the lanes of that depth take the places behind it in lane order.
__global__ __launch_bounds__(kReanchorBlock) void k_reanchor_scatter(const int* __restrict__ hop, int rows,
                                                                     int* __restrict__ cursor, int* __restrict__ order) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kReanchorBlock;
    for (long long base = (long long)blockIdx.x * kReanchorBlock; base < rows; base += stride) {   // uniform
        const long long row = base + threadIdx.x;
        const bool in = row < rows;
        const int h = in ? hop[row] : -1;
        unsigned long long todo = __ballot(in);
        while (todo) {   // uniform
            const int leader = (int)__builtin_ctzll(todo);
            const int v = __builtin_amdgcn_readlane(h, leader);
            const unsigned long long same = __ballot(h == v);
            int first = 0;
            if (lane == leader) first = atomicAdd(&cursor[v], (int)__popcll(same));
            first = __builtin_amdgcn_readlane(first, leader);
            if (h == v) order[(long long)first + (long long)__popcll(same & ((1ull << lane) - 1ull))] = (int)row;
            todo &= ~same;
        }
    }
}

// The rows order[begin .. end) of one level.  top: level 0, whose rows are row 0 (the new root
// state) and the orphans.  Below it every row has a usable parent one level up, whose alive
// byte and output state the launch before wrote.  out and alive are read (the parent's) and
// written (the row's) by this launch, at different rows.
template <int AGENT, int OBS>
__global__ __launch_bounds__(kReanchorBlock) void k_reanchor_level(KgmtDev d, const int* __restrict__ order,
                                                                   unsigned begin, unsigned end, int top, float4 s0,
                                                                   float4* out, uint8_t* alive,
                                                                   uint8_t* __restrict__ status,
                                                                   ReanchorAcc* __restrict__ acc) {
    extern __shared__ float4 sObs[];
    __shared__ unsigned sAcc[5];
    constexpr bool kLdsObs = (OBS == kObsLds || OBS == kObsLds4);
    constexpr int kRegObs = obs_in_registers(OBS);
    if (threadIdx.x < 5) sAcc[threadIdx.x] = threadIdx.x == 4 ? ~0u : 0u;
    unsigned nAlive = 0, nBlocked = 0, nOrphan = 0, nCut = 0, first = ~0u;
    // unsigned: end <= rows < 2^31 and a sweep is at most 2^19 rows, so i + stride cannot wrap
    const unsigned stride = gridDim.x * kReanchorBlock;
    const float4* tState = d.treeState;
    if (top) {   // uniform
        __syncthreads();
        for (unsigned i = begin + blockIdx.x * kReanchorBlock + threadIdx.x; i < end; i += stride) {
            const int r = order[i];
            const bool root = r == 0;
            out[r] = root ? s0 : tState[r];
            alive[r] = root ? 1 : 0;
            status[r] = root ? SBMP_ROW_FREE : SBMP_ROW_ORPHAN;
            nAlive += root;
            nOrphan += !root;
            if (!root && (unsigned)r < first) first = (unsigned)r;
        }
    } else {
        float4 ro[kRegObs > 0 ? kRegObs : 1];   // register-resident obstacle list
#pragma unroll
        for (int i = 0; i < kRegObs; ++i) {
            ro[i] = d.obstacles[i];
            // in vector registers, as k_tree_recheck holds them (tree_recheck.hip)
            asm volatile("" : "+v"(ro[i].x), "+v"(ro[i].y), "+v"(ro[i].z), "+v"(ro[i].w));
        }
        if (kLdsObs)
            for (int i = threadIdx.x; i < d.nObs; i += kReanchorBlock) sObs[i] = d.obstacles[i];
        __syncthreads();
        const float4* obs = (kRegObs > 0) ? ro : kLdsObs ? sObs : d.obstacles;
        // the row loop's pointers in vector registers, for the same reason
        const float4* tCtrl = d.treeCtrl;
        const int* tParent = d.treeParent;
        asm volatile("" : "+v"(status), "+v"(out), "+v"(alive), "+v"(tState), "+v"(tCtrl), "+v"(tParent), "+v"(order));
        for (unsigned i = begin + blockIdx.x * kReanchorBlock + threadIdx.x; i < end; i += stride) {
            const int r = order[i];
            const int parent = tParent[r];   // usable: the row has depth >= 1
            const bool parentAlive = alive[parent] != 0;
            bool valid = false;
            ChildOut o;
            if (parentAlive) {
                const float4 p = out[parent];
                const float4 c = tCtrl[r];
                const ChildCtl ctl = stored_controls<AGENT>(c, d);
                valid = (AGENT == 0) ? car_euler<OBS>(p, ctl, d, obs, o) : point_euler<OBS>(p, ctl, d, obs, o);
            }
            const uint8_t st = reanchor_status(parentAlive, valid);
            if (st == SBMP_ROW_FREE) out[r] = o.state;
            else out[r] = tState[r];
            alive[r] = st == SBMP_ROW_FREE ? 1 : 0;
            status[r] = st;
            nAlive += st == SBMP_ROW_FREE;
            nBlocked += st == SBMP_ROW_BLOCKED;
            nCut += st == (SBMP_ROW_FREE | SBMP_ROW_CUT);
            if (st != SBMP_ROW_FREE && (unsigned)r < first) first = (unsigned)r;
        }
    }
    if (nAlive) atomicAdd(&sAcc[0], nAlive);
    if (nBlocked) atomicAdd(&sAcc[1], nBlocked);
    if (nOrphan) atomicAdd(&sAcc[2], nOrphan);
    if (nCut) atomicAdd(&sAcc[3], nCut);
    if (first != ~0u) atomicMin(&sAcc[4], first);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sAcc[0]) atomicAdd(&acc->alive, sAcc[0]);
        if (sAcc[1]) atomicAdd(&acc->blocked, sAcc[1]);
        if (sAcc[2]) atomicAdd(&acc->orphan, sAcc[2]);
        if (sAcc[3]) atomicAdd(&acc->cut, sAcc[3]);
        if (sAcc[4] != ~0u) atomicMin(&acc->firstDead, sAcc[4]);
    }
}

// ---------------------------------------------------------------- host side
template <class Kernel>
int reanchor_grid(Kernel* fn, long long lanes, const char* name) {
    return resident_grid(fn, kReanchorBlock, 0, kReanchorGroupsPerCU, lanes, name);
}

using ReanchorFn = decltype(&k_reanchor_level<0, kObsGlobal>);

// ceil(log2(bound)): after that many passes hop[r] covers 2^passes >= bound edges of r's chain.
int reanchor_jump_passes(long long bound) {
    int p = 0;
    while ((1ll << p) < bound) ++p;
    return p;
}

void check_reanchor_root(const float* s0) {
    if (!s0) throw Error(SBMP_ERR_INVALID_ARGUMENT, "newRoot must be non-NULL");
    if (!reanchor_root_finite(s0[0], s0[1], s0[2], s0[3]))
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "newRoot must be four finite floats (x, y, theta, v)");
}

void check_reanchor_args(const sbmp_tree_recheck_args* a, const float* s0, const sbmp_tree_reanchor* out) {
    if (!a || !out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "args and out must be non-NULL");
    if (!a->state || !a->ctrl || !a->parent) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and parent must be non-NULL");
    if (a->rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    if (a->numDisc < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "numDisc must be >= 1");
    if (a->obstaclesCount < 0 || (a->obstaclesCount > 0 && !a->obstacles))
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad obstacle list");
    if (a->agent != SBMP_AGENT_CAR && a->agent != SBMP_AGENT_POINT) throw Error(SBMP_ERR_INVALID_ARGUMENT, "agent");
    check_reanchor_root(s0);
}
}  // namespace

void tree_reanchor_device(const KgmtDev& base, int agent, int variant, int rows, int depthBound, const float* newRoot,
                          const float* d_obstacles, int nObs, float* d_outState, uint8_t* d_alive, uint8_t* status,
                          sbmp_tree_reanchor* out, hipStream_t stream) {
    if (rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    if (nObs < 0 || (nObs > 0 && !d_obstacles)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad obstacle list");
    if (!out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "out must be non-NULL");
    check_reanchor_root(newRoot);
    KgmtDev d = base;   // the plan's own struct, list and grid stay untouched
    DevBufs listBufs, w;   // freed with the call: the scratch first, then the list
    ReanchorAcc acc;
    int levels = 0;
    drained_on_throw(stream, [&] {
        attach_list(listBufs, d, d_obstacles, nObs, variant, stream);
        const int passes = std::max(1, reanchor_jump_passes(depthBound > 0 ? std::min(depthBound, rows) : rows));
        // a depth is < rows, and <= 2^passes once the jumps are done
        const int depths = (int)std::min<long long>(rows, (1ll << passes) + 1);
        int* anc[2] = {w.alloc<int>((size_t)rows), w.alloc<int>((size_t)rows)};
        int* hop[2] = {w.alloc<int>((size_t)rows), w.alloc<int>((size_t)rows)};
        int* count = w.alloc<int>((size_t)depths);
        int* cursor = w.alloc<int>((size_t)depths);
        int* meta = w.alloc<int>((size_t)kReanchorMeta + depths + 1);
        int* off = meta + kReanchorMeta;
        int* order = w.alloc<int>((size_t)rows);
        uint8_t* dStatus = w.alloc<uint8_t>((size_t)rows);
        ReanchorAcc* dAcc = w.alloc<ReanchorAcc>(1);
        float4* dOut = d_outState ? reinterpret_cast<float4*>(d_outState) : w.alloc<float4>((size_t)rows);
        uint8_t* dAlive = d_alive ? d_alive : w.alloc<uint8_t>((size_t)rows);
        SBMP_HIP(hipMemsetAsync(count, 0, sizeof(int) * (size_t)depths, stream));
        SBMP_HIP(hipMemsetAsync(meta, 0, sizeof(int) * kReanchorMeta, stream));
        SBMP_HIP(hipMemsetAsync(dAcc, 0, sizeof(ReanchorAcc), stream));
        SBMP_HIP(hipMemsetAsync(&dAcc->firstDead, 0xff, sizeof(unsigned), stream));

        const int* tParent = d.treeParent;
        hipLaunchKernelGGL(k_reanchor_init, dim3(reanchor_grid(k_reanchor_init, rows, "k_reanchor_init")),
                           dim3(kReanchorBlock), 0, stream, tParent, rows, anc[0], hop[0]);
        // pass p reads pair p & 1 and writes pair (p + 1) & 1
        const int gridJump = reanchor_grid(k_reanchor_jump, rows, "k_reanchor_jump");
        for (int p = 0; p < passes; ++p)
            hipLaunchKernelGGL(k_reanchor_jump, dim3(gridJump), dim3(kReanchorBlock), 0, stream, (const int*)anc[p & 1],
                               (const int*)hop[p & 1], anc[(p + 1) & 1], hop[(p + 1) & 1], rows);
        const int* ancF = anc[passes & 1];
        const int* hopF = hop[passes & 1];
        hipLaunchKernelGGL(k_reanchor_hist, dim3(reanchor_grid(k_reanchor_hist, rows, "k_reanchor_hist")),
                           dim3(kReanchorBlock), 0, stream, ancF, hopF, rows, depths, count, meta);
        hipLaunchKernelGGL(k_reanchor_offsets, dim3(1), dim3(kReanchorBlock), 0, stream, (const int*)count, depths, off,
                           cursor, meta);
        hipLaunchKernelGGL(k_reanchor_scatter, dim3(reanchor_grid(k_reanchor_scatter, rows, "k_reanchor_scatter")),
                           dim3(kReanchorBlock), 0, stream, hopF, rows, cursor, order);
        SBMP_HIP(hipGetLastError());
        // the one wait before the levels: the flag, the level count and the offsets
        std::vector<int> h((size_t)kReanchorMeta + depths + 1);
        read_back(stream, {{h.data(), meta, sizeof(int) * h.size()}});
        if (h[0] != 0)
            throw Error(SBMP_ERR_INVALID_ARGUMENT, "depthBound " + std::to_string(depthBound) +
                                                       " is below the rows of the longest parent chain: a level would "
                                                       "read a parent's state before it is written");
        levels = h[1];
        const int* hOff = h.data() + kReanchorMeta;
        if (levels < 1 || levels > depths || hOff[levels] != rows)
            throw Error(SBMP_ERR_HIP, "reanchor: the level offsets do not cover the rows");

        const float4 s0 = make_float4(newRoot[0], newRoot[1], newRoot[2], newRoot[3]);
        with_obs_form(d, variant, [&](auto obs) {
            const ReanchorFn fn = (agent == SBMP_AGENT_POINT) ? k_reanchor_level<1, obs.value> : k_reanchor_level<0, obs.value>;
            const size_t lds = (obs.value == kObsLds || obs.value == kObsLds4) ? sizeof(float4) * (size_t)d.nObs : 0;
            // what the device holds at once of fn, asked once; a level takes no more than it needs
            const int resident = resident_grid(fn, kReanchorBlock, lds, kReanchorGroupsPerCU, kWholeDevice, "k_reanchor_level");
            for (int lv = 0; lv < levels; ++lv) {
                const int begin = hOff[lv], end = hOff[lv + 1];
                if (end <= begin) continue;
                const long long need = ((long long)(end - begin) + kReanchorBlock - 1) / kReanchorBlock;
                const int grid = (int)std::min<long long>(resident, need);
                hipLaunchKernelGGL(fn, dim3(grid), dim3(kReanchorBlock), lds, stream, d, (const int*)order, (unsigned)begin,
                                   (unsigned)end, lv == 0 ? 1 : 0, s0, dOut, dAlive, dStatus, dAcc);
            }
        });
        SBMP_HIP(hipGetLastError());
        read_back(stream, {{&acc, dAcc, sizeof(acc)}, {status, dStatus, (size_t)rows}});
    });
    out->rows = rows;
    out->alive = (int)acc.alive;
    out->blocked = (int)acc.blocked;
    out->orphan = (int)acc.orphan;
    out->cut = (int)acc.cut;
    out->firstDead = acc.firstDead == ~0u ? -1 : (int)acc.firstDead;
    out->levels = levels;
}

void tree_reanchor_batch(const sbmp_tree_recheck_args* a, const float* newRoot, float* d_outState, uint8_t* d_alive,
                         uint8_t* status, sbmp_tree_reanchor* out, hipStream_t stream) {
    check_reanchor_args(a, newRoot, out);
    KgmtDev d{};
    set_euler_params(d, a->numDisc, a->agentLength);
    d.width = a->width;
    d.height = a->height;
    d.treeState = reinterpret_cast<float4*>(const_cast<float*>(a->state));
    d.treeCtrl = reinterpret_cast<float4*>(const_cast<float*>(a->ctrl));
    d.treeParent = const_cast<int*>(a->parent);
    tree_reanchor_device(d, a->agent, expand_variant_from_env(), a->rows, a->depthBound, newRoot, a->obstacles,
                         a->obstaclesCount, d_outState, d_alive, status, out, stream);
}

void tree_reanchor_batch_host(const sbmp_tree_recheck_args* a, const float* newRoot, float* outState, uint8_t* alive,
                              uint8_t* status, sbmp_tree_reanchor* out) {
    check_reanchor_args(a, newRoot, out);
    std::vector<float> ownState;
    std::vector<uint8_t> ownAlive;
    if (!outState) {
        ownState.resize(4 * (size_t)a->rows);
        outState = ownState.data();
    }
    if (!alive) {
        ownAlive.resize((size_t)a->rows);
        alive = ownAlive.data();
    }
    reanchor_rows_host(a->state, a->ctrl, a->parent, a->rows, newRoot, a->agent, a->numDisc, a->agentLength, a->width,
                       a->height, a->obstacles, a->obstaclesCount, outState, alive, status, out);
}

}  // namespace sbmp

// tree_adopt.hip — a tree adopted into a planner as its iteration 1 (include/sbmp/tree_adopt.h
// states the rule).
//   k_adopt_scan     one lane per row: the row's two cells into scratch, its class (non-finite,
//                    non-finite inside the frontier, out of grid, inside the goal), a ballot and a
//                    population count per wave, the wave's lowest goal row, one atomic per
//                    workgroup and field.  Reads the caller's rows only: the host refuses on the
//                    summary before any planner buffer is touched
//   k_adopt_seed     the rows into treeState / treeCtrl / treeParent (a streaming copy, 36 bytes a
//                    row), the R1 histogram in LDS with one global add per non-zero cell and
//                    workgroup, the R2 bits with one atomicOr per distinct cell of a wave (the
//                    lowest lane that holds it)
//   k_adopt_tables   one workgroup: R1Valid = R1, R1Avail = R1 > 0, R1Invalid = 0, R1Cov by
//                    population count over each cell's R2 bits, both parities, ctrl[1], status
//   sbmp_tree_adopt_tables / _host, and the two stages KgmtPlanner::adopt_tree runs round begin()'s
//   clears (kgmt_planner.cpp)
// Stream order between the launches is the only ordering.  Every decision is an integer one and
// the tables are integer adds and ors, so the bytes do not depend on the grid or on the order
// rows arrive in.  Row indices are 32-bit; every byte offset (16 x row) is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_adopt.h"
#include "tree_pass.h"

namespace sbmp {

namespace {
constexpr int kAdoptBlock = 256;       // lanes per workgroup
constexpr int kAdoptGroupsPerCU = 8;   // as the other streaming passes
static_assert(kAdoptMaxR1 <= kAdoptBlock, "one R1 cell per lane");

struct AdoptGrid {
    float R1Size, R2Size;
    int N, n;
    float goal[3];
    int hasGoal;
};

// The summary's accumulators (device), zeroed before the scan.  goalInv: 0 for no goal row, else
// 0xffffffff - row, so the lowest row is the maximum and a memset is the initial value.
struct AdoptAcc {
    unsigned nonFinite, frontierNonFinite, outOfGrid, goalInv;
};
__host__ __device__ inline int adopt_goal_row(unsigned goalInv) { return goalInv ? (int)(0xffffffffu - goalInv) : -1; }

__global__ __launch_bounds__(kAdoptBlock) void k_adopt_scan(const float4* __restrict__ state, long long rows,
                                                            long long frontierFrom, AdoptGrid g,
                                                            int2* __restrict__ cells, AdoptAcc* __restrict__ acc) {
    __shared__ unsigned sAcc[4];
    if (threadIdx.x < 4) sAcc[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned nNonFinite = 0u, nFrontier = 0u, nOut = 0u, goalInv = 0u;   // wave-uniform
    const long long stride = (long long)gridDim.x * kAdoptBlock;
    for (long long base = (long long)blockIdx.x * kAdoptBlock; base < rows; base += stride) {   // uniform
        const long long row = base + threadIdx.x;
        bool nonFinite = false, inFrontier = false, outOfGrid = false, inGoal = false;
        if (row < rows) {
            const float4 s = state[row];
            int r1, r2;
            adopt_row_cells(s.x, s.y, g.R1Size, g.N, g.R2Size, g.n, &r1, &r2);
            cells[row] = make_int2(r1, r2);
            nonFinite = !adopt_row_finite(s.x, s.y, s.z, s.w);
            inFrontier = nonFinite && adopt_row_in_frontier(row, frontierFrom);
            outOfGrid = adopt_row_out_of_grid(r1, r2);
            inGoal = adopt_row_in_goal(s.x, s.y, g.hasGoal ? g.goal : nullptr);
        }
        nNonFinite += (unsigned)__popcll(__ballot(nonFinite));
        nFrontier += (unsigned)__popcll(__ballot(inFrontier));
        nOut += (unsigned)__popcll(__ballot(outOfGrid));
        const unsigned long long gb = __ballot(inGoal);
        // rows grow with the lane and with the round: the first one a wave meets is its lowest
        if (gb && !goalInv) goalInv = 0xffffffffu - (unsigned)(row - lane + (long long)__builtin_ctzll(gb));
    }
    if (lane == 0) {
        if (nNonFinite) atomicAdd(&sAcc[0], nNonFinite);
        if (nFrontier) atomicAdd(&sAcc[1], nFrontier);
        if (nOut) atomicAdd(&sAcc[2], nOut);
        if (goalInv) atomicMax(&sAcc[3], goalInv);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sAcc[0]) atomicAdd(&acc->nonFinite, sAcc[0]);
        if (sAcc[1]) atomicAdd(&acc->frontierNonFinite, sAcc[1]);
        if (sAcc[2]) atomicAdd(&acc->outOfGrid, sAcc[2]);
        if (sAcc[3]) atomicMax(&acc->goalInv, sAcc[3]);
    }
}

// dState null: the tables alone (sbmp_tree_adopt_tables).  R1: nR1 ints and R2bits: the bit words,
// both zero before the launch.  A cell of the scratch is a cell of the grid or -1 (k_adopt_scan).
__global__ __launch_bounds__(kAdoptBlock) void k_adopt_seed(const float4* __restrict__ sState,
                                                            const float4* __restrict__ sCtrl,
                                                            const int* __restrict__ sParent,
                                                            const int2* __restrict__ cells, long long rows,
                                                            float4* __restrict__ dState, float4* __restrict__ dCtrl,
                                                            int* __restrict__ dParent, int* __restrict__ R1,
                                                            uint32_t* __restrict__ R2bits, int nR1) {
    __shared__ int sHist[kAdoptMaxR1];
    sHist[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * kAdoptBlock;
    for (long long base = (long long)blockIdx.x * kAdoptBlock; base < rows; base += stride) {   // uniform
        const long long row = base + threadIdx.x;
        int r1 = -1, r2 = -1;
        if (row < rows) {
            const int2 c = cells[row];
            r1 = c.x;
            r2 = c.y;
            if (dState) {
                const float4 s = sState[row], u = sCtrl[row];
                const int p = sParent[row];
                dState[row] = s;
                dCtrl[row] = u;
                dParent[row] = p;
            }
        }
        if (r1 >= 0) atomicAdd(&sHist[r1], 1);
        // A bit that is already set needs no atomic: every lane looks first (a load at the device's
        // coherence point; 2^24 rows share at most 2,048 words, and read-modify-writes on one word
        // serialise there).  A stale 0 only costs one atomicOr more.
        bool need = false;
        if (r2 >= 0) {
            const uint32_t have = __hip_atomic_load(&R2bits[r2 >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            need = ((have >> (r2 & 31)) & 1u) == 0u;
        }
        // one atomicOr per distinct cell of the wave that still needs one, by the lowest lane that holds it
        unsigned long long todo = __ballot(need);
        while (todo) {   // uniform
            const int leader = (int)__builtin_ctzll(todo);
            const int v = __builtin_amdgcn_readlane(r2, leader);
            const unsigned long long same = __ballot(r2 == v);
            if (lane == leader) atomicOr(&R2bits[v >> 5], 1u << (v & 31));
            todo &= ~same;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nR1 && sHist[threadIdx.x]) atomicAdd(&R1[threadIdx.x], sHist[threadIdx.x]);
}

// tab: [2 parities][R1, R1Avail, R1Valid, R1Invalid, R1Cov][nR1] with the histogram in parity 0's
// R1; bits: [2 parities][nW] with parity 0 set.  ctrl1 / status: the planner's ctrl[1] and status
// block, or null.
__global__ __launch_bounds__(kAdoptBlock) void k_adopt_tables(int* __restrict__ tab, uint32_t* bits, int nR1, int nn,
                                                              int nW, IterCtrl* __restrict__ ctrl1,
                                                              PlannerStatus* __restrict__ status,
                                                              const AdoptAcc* __restrict__ acc, int rows,
                                                              int frontierFrom) {
    const int c = (int)threadIdx.x;
    if (c < nR1) {
        const int r1 = tab[c];
        const int cov = adopt_cell_cov(bits, c, nn);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int* t = tab + (size_t)p * 5 * nR1;
            t[c] = r1;
            t[nR1 + c] = r1 > 0 ? 1 : 0;
            t[2 * nR1 + c] = r1;
            t[3 * nR1 + c] = 0;
            t[4 * nR1 + c] = cov;
        }
    }
    for (int w = c; w < nW; w += kAdoptBlock) bits[(size_t)nW + w] = bits[w];
    if (c == 0 && ctrl1) {
        const AdoptCtrl a = adopt_ctrl(rows, frontierFrom);
        IterCtrl k{};
        k.run = a.run;
        k.executed = a.executed;
        k.treeSize = a.treeSize;
        k.gLo = a.gLo;
        k.nG = a.nG;
        k.k = a.k;
        k.nExp = a.nExp;
        k.S = a.S;
        k.H = a.H;
        k.A = a.A;
        k.scoreBuf = 1;   // the buffer an iteration 1 uses
        *ctrl1 = k;
    }
    if (c == 0 && status) {
        const int g = adopt_goal_row(acc->goalInv);
        status->goalIdx = g < 0 ? kNoGoal : g;
        status->error = 0;
    }
}

template <class Kernel>
int adopt_grid(Kernel* fn, long long lanes, const char* name) {
    return resident_grid(fn, kAdoptBlock, 0, kAdoptGroupsPerCU, lanes, name);
}

AdoptGrid adopt_grid_of(float width, int N, int n, const float* goal) {
    AdoptGrid g{};
    g.R1Size = adopt_r1_size(width, N);
    g.R2Size = adopt_r2_size(width, N, n);
    g.N = N;
    g.n = n;
    g.hasGoal = goal ? 1 : 0;
    for (int i = 0; i < 3; ++i) g.goal[i] = goal ? goal[i] : 0.0f;
    return g;
}

void scan_rows(const float4* dState, long long rows, long long frontierFrom, const AdoptGrid& g, int2* cells,
               AdoptAcc* dAcc, sbmp_tree_adopt* out, hipStream_t stream) {
    SBMP_HIP(hipMemsetAsync(dAcc, 0, sizeof(AdoptAcc), stream));
    hipLaunchKernelGGL(k_adopt_scan, dim3(adopt_grid(k_adopt_scan, rows, "k_adopt_scan")), dim3(kAdoptBlock), 0, stream,
                       dState, rows, frontierFrom, g, cells, dAcc);
    SBMP_HIP(hipGetLastError());
    AdoptAcc acc;
    read_back(stream, {{&acc, dAcc, sizeof(acc)}});
    sbmp_tree_adopt s{};
    s.rows = (int)rows;
    s.nonFinite = (int)acc.nonFinite;
    s.frontierNonFinite = (int)acc.frontierNonFinite;
    s.outOfGrid = (int)acc.outOfGrid;
    s.goalRow = adopt_goal_row(acc.goalInv);
    s.treeSize = (int)rows;
    s.gLo = (int)frontierFrom;
    *out = s;
}

void check_tables_args(const sbmp_tree_adopt_tables_args* a, const sbmp_tree_adopt* out) {
    if (!a || !out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "args and out must be non-NULL");
    if (!a->state) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state must be non-NULL");
    if (a->rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    if (a->frontierFrom < 0 || a->frontierFrom > a->rows)
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "frontierFrom " + std::to_string(a->frontierFrom) + " is outside [0, " +
                                                   std::to_string(a->rows) + "]");
    if (!(a->width > 0.0f) || !std::isfinite(a->width)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "width must be > 0");
    if (a->N < 1 || a->N * a->N > kAdoptMaxR1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "N * N must be in [1, 256]");
    if (a->n < 1 || a->n > kAdoptMaxN2) throw Error(SBMP_ERR_INVALID_ARGUMENT, "n must be in [1, 16]");
    if (a->goal)
        for (int i = 0; i < 2; ++i)
            if (!std::isfinite(a->goal[i])) throw Error(SBMP_ERR_INVALID_ARGUMENT, "the goal's x and y must be finite");
}
}  // namespace

size_t tree_adopt_scratch_bytes(int rows) { return sizeof(int2) * (size_t)rows + 256; }

// The scan of an adoption into a planner: the cells of every row into `scratch`
// (tree_adopt_scratch_bytes(rows) bytes: the accumulators, then the cells) and the summary to
// the host.  Waits for the result; touches nothing of the planner.
void tree_adopt_scan(const KgmtDev& d, const float* d_state, int rows, int frontierFrom, const float* goalXY,
                     void* scratch, sbmp_tree_adopt* out, hipStream_t stream) {
    const float goal[3] = {goalXY[0], goalXY[1], d.goalThreshold};
    AdoptAcc* dAcc = static_cast<AdoptAcc*>(scratch);
    int2* cells = reinterpret_cast<int2*>(static_cast<char*>(scratch) + 256);
    scan_rows(reinterpret_cast<const float4*>(d_state), rows, frontierFrom, adopt_grid_of(d.width, d.N, d.n, goal), cells,
              dAcc, out, stream);
}

// The adoption itself, queued on `stream` behind begin()'s clears: the rows into the tree, the
// histogram and the bits into parity 0, then both parities, ctrl[1] and status.  No wait.
void tree_adopt_seed(const KgmtDev& d, const float* d_state, const float* d_ctrl, const int* d_parent, int rows,
                     int frontierFrom, const void* scratch, hipStream_t stream) {
    const AdoptAcc* dAcc = static_cast<const AdoptAcc*>(scratch);
    const int2* cells = reinterpret_cast<const int2*>(static_cast<const char*>(scratch) + 256);
    hipLaunchKernelGGL(k_adopt_seed, dim3(adopt_grid(k_adopt_seed, rows, "k_adopt_seed")), dim3(kAdoptBlock), 0, stream,
                       reinterpret_cast<const float4*>(d_state), reinterpret_cast<const float4*>(d_ctrl), d_parent, cells,
                       (long long)rows, d.treeState, d.treeCtrl, d.treeParent, d.R1, d.R2Avail, d.nR1);
    hipLaunchKernelGGL(k_adopt_tables, dim3(1), dim3(kAdoptBlock), 0, stream, d.R1, d.R2Avail, d.nR1, d.n * d.n,
                       d.nR2 / 32, d.ctrl + 1, d.status, dAcc, rows, frontierFrom);
    SBMP_HIP(hipGetLastError());
}

void tree_adopt_tables_device(const sbmp_tree_adopt_tables_args* a, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid,
                              int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out, hipStream_t stream) {
    check_tables_args(a, out);
    const int nR1 = a->N * a->N, nn = a->n * a->n, nW = adopt_r2_words(a->N, a->n);
    DevBufs w;
    drained_on_throw(stream, [&] {
        int* tab = w.alloc<int>((size_t)2 * 5 * nR1);
        uint32_t* bits = w.alloc<uint32_t>((size_t)2 * nW);
        int2* cells = w.alloc<int2>((size_t)a->rows);
        AdoptAcc* dAcc = w.alloc<AdoptAcc>(1);
        SBMP_HIP(hipMemsetAsync(tab, 0, sizeof(int) * 2 * 5 * nR1, stream));
        SBMP_HIP(hipMemsetAsync(bits, 0, sizeof(uint32_t) * 2 * nW, stream));
        const float4* st = reinterpret_cast<const float4*>(a->state);
        scan_rows(st, a->rows, a->frontierFrom, adopt_grid_of(a->width, a->N, a->n, a->goal), cells, dAcc, out, stream);
        hipLaunchKernelGGL(k_adopt_seed, dim3(adopt_grid(k_adopt_seed, a->rows, "k_adopt_seed")), dim3(kAdoptBlock), 0,
                           stream, st, (const float4*)nullptr, (const int*)nullptr, (const int2*)cells, (long long)a->rows,
                           (float4*)nullptr, (float4*)nullptr, (int*)nullptr, tab, bits, nR1);
        hipLaunchKernelGGL(k_adopt_tables, dim3(1), dim3(kAdoptBlock), 0, stream, tab, bits, nR1, nn, nW,
                           (IterCtrl*)nullptr, (PlannerStatus*)nullptr, (const AdoptAcc*)dAcc, a->rows, a->frontierFrom);
        SBMP_HIP(hipGetLastError());
        // the second parity is what the caller gets: the copy is part of what is checked
        const int* t1 = tab + (size_t)5 * nR1;
        read_back(stream, {{R1, t1, sizeof(int) * nR1},
                           {R1Avail, t1 + nR1, sizeof(int) * nR1},
                           {R1Valid, t1 + 2 * nR1, sizeof(int) * nR1},
                           {R1Invalid, t1 + 3 * nR1, sizeof(int) * nR1},
                           {R1Cov, t1 + 4 * nR1, sizeof(int) * nR1},
                           {R2bits, bits + nW, sizeof(uint32_t) * nW}});
    });
}

void tree_adopt_tables_host(const sbmp_tree_adopt_tables_args* a, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid,
                            int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out) {
    check_tables_args(a, out);
    adopt_tables_host(a->state, a->rows, a->frontierFrom, a->width, a->N, a->n, a->goal, R1, R1Avail, R1Valid, R1Invalid,
                      R1Cov, R2bits, out);
}

}  // namespace sbmp

// tree_query.hip — goal queries against a grown tree (include/sbmp/tree_query.h states the
// rule): for each goal disc, how many rows lie inside, the lowest of them,
// the cheapest of them, and the row nearest to the centre.
//   k_tree_query             one streaming pass over the rows for a tile of up to 16 goals
//   sbmp_tree_query_batch    the kernel over caller rows (tree_query_device)
//   sbmp_tree_query_batch_host   a plain host loop with the literal rule (tree_query_host)
//   sbmp_kgmt_query_goals    the kernel over a planner's tree (KgmtPlanner::query_goals)
// The kernel reads treeState once, 16 B per row; a row's cost (treeCtrl.w) is read only by
// a lane whose row is inside some disc.  Every reduction is an integer add or an unsigned
// minimum (of a row, or of goal_key = value bits << 32 | row), so the answer does not
// depend on the order rows arrive in: it is the same bits on every run, whatever the grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_query.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

namespace {
constexpr int kQueryBlock = 256;   // lanes per workgroup
constexpr int kQueryRows = 8;      // rows per lane in flight
constexpr int kQueryChunk = kQueryBlock * kQueryRows;   // rows a workgroup takes per step
// Workgroups per CU the grid is sized for, at most (the occupancy query may give fewer).
// One sweep of the grid is therefore at most CUs x 8 x 2,048 rows: 4,194,304 rows on
// the 256 CUs of an MI355X; longer trees go round the grid-stride loop again.
constexpr int kQueryGroupsPerCU = 8;

// A tile of NG goals as a kernel argument: the centres and thresholds arrive in SGPRs
// (kernel-argument loads are scalar), and the loops over them unroll.
template <int NG>
struct QueryTile {
    float gx[NG], gy[NG], t[NG];
};

__global__ void k_tree_query_init(QueryAcc* acc, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        acc[i].best = kNoGoalKey;
        acc[i].nearest = kNoGoalKey;
        acc[i].count = 0u;
        acc[i].first = ~0u;
    }
}

// if (b < nb) { nb = b; nr = row; } as one compare into VCC and the two selects that read it,
// kept together.  Written as C++, nb became a v_min_u32 and every comparison's lane mask was
// parked in an SGPR pair for a row select scheduled much later: 128 live masks per step, which
// the 16-goal kernel spilled to VGPR lanes (two v_writelane and two v_readlane per pair).
__device__ __forceinline__ void keep_lower(uint32_t& nb, uint32_t& nr, uint32_t b, uint32_t row) {
    asm("v_cmp_lt_u32_e32 vcc, %2, %0\n\tv_cndmask_b32_e32 %0, %0, %2, vcc\n\tv_cndmask_b32_e32 %1, %1, %3, vcc"
        : "+v"(nb), "+v"(nr)
        : "v"(b), "v"(row)
        : "vcc");
}

// The rows base + u * kQueryBlock, u < kQueryRows, of one lane (TAIL: some may lie at or
// past `rows`).  All loads are issued before the first use.  nb / nr: the lane's running
// minimum of d2 (as bits) per goal and its row; a lane meets its rows in ascending order, so
// the strict comparison keeps the lowest row of equal d2.
template <int NG, bool TAIL>
__device__ __forceinline__ void query_rows(const float4* __restrict__ state, const float4* __restrict__ ctrl,
                                           long long rows, long long base, const QueryTile<NG>& q, uint32_t (&nb)[NG],
                                           uint32_t (&nr)[NG], const float* sGoal, unsigned* sCount,
                                           unsigned* sFirst, unsigned long long* sBest) {
    float px[kQueryRows], py[kQueryRows];
#pragma unroll
    for (int u = 0; u < kQueryRows; ++u) {
        const long long row = base + (long long)u * kQueryBlock;   // 64-bit: rows x 16 B may pass 2^31
        px[u] = 0.0f;
        py[u] = 0.0f;
        if (!TAIL || row < rows) {
            const float4 s = state[row];
            px[u] = s.x;
            py[u] = s.y;
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // every load issued before the first row is used
    // slack = max over this lane's (row, goal) pairs of t - d2: a pair is inside iff d2 <= t,
    // and then t - d2 >= 0 (the sign of an IEEE difference is exact; a NaN d2 is skipped by
    // the max), so slack < 0 proves that no pair is.  One subtract and one max on the vector
    // unit per pair, where the comparisons' lane masks, OR-ed on the scalar unit, ran the
    // kernel out of SGPRs.  The rows behind slack >= 0 are tested again, exactly, below.
    float slack = -1.0f;
#pragma unroll
    for (int u = 0; u < kQueryRows; ++u) {
        const long long row = base + (long long)u * kQueryBlock;
        const bool live = !TAIL || row < rows;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float d2 = goal_d2(px[u], py[u], q.gx[g], q.gy[g]);
            slack = __builtin_fmaxf(slack, q.t[g] - d2);
            // d2 >= 0: the bits order as the values; a row past the end never wins
            const uint32_t b = live ? __float_as_uint(d2) : ~0u;
            keep_lower(nb[g], nr[g], b, (uint32_t)row);
        }
    }
    // Rare: some row of this lane may be inside some disc.  The rows are read again (they are
    // in L2), so the code above keeps its rows in registers that nothing indexes.
    if (slack >= 0.0f) {
#pragma unroll 1
        for (int u = 0; u < kQueryRows; ++u) {
            const long long row = base + (long long)u * kQueryBlock;
            if (TAIL && row >= rows) break;
            const float4 s = state[row];
#pragma unroll 1
            for (int g = 0; g < NG; ++g) {   // the tile's copy in LDS: a rolled loop cannot index SGPRs
                if (!(goal_d2(s.x, s.y, sGoal[g], sGoal[NG + g]) <= sGoal[2 * NG + g])) continue;
                atomicAdd(&sCount[g], 1u);
                atomicMin(&sFirst[g], (unsigned)row);
                atomicMin(&sBest[g], goal_key(ctrl[row].w, (uint32_t)row));
            }
        }
    }
}

// acc: the accumulators of this tile's first goal; n <= NG goals of the tile are real (the
// rest are padding with t = -1, whose results are dropped).
template <int NG>
__global__ __launch_bounds__(kQueryBlock) void k_tree_query(const float4* __restrict__ state,
                                                            const float4* __restrict__ ctrl, long long rows,
                                                            QueryTile<NG> q, int n, QueryAcc* __restrict__ acc) {
    __shared__ unsigned sCount[NG], sFirst[NG];
    __shared__ unsigned long long sBest[NG], sNear[NG];
    __shared__ float sGoal[3 * NG];   // gx | gy | t, for the rare rows that are inside a disc
    if (threadIdx.x < NG) {
        sGoal[threadIdx.x] = q.gx[threadIdx.x];
        sGoal[NG + threadIdx.x] = q.gy[threadIdx.x];
        sGoal[2 * NG + threadIdx.x] = q.t[threadIdx.x];
        sCount[threadIdx.x] = 0u;
        sFirst[threadIdx.x] = ~0u;
        sBest[threadIdx.x] = kNoGoalKey;
        sNear[threadIdx.x] = kNoGoalKey;
    }
    __syncthreads();
    uint32_t nb[NG], nr[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        nb[g] = ~0u;
        nr[g] = ~0u;
    }
    const long long full = rows / kQueryChunk, chunks = (rows + kQueryChunk - 1) / kQueryChunk;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long base = c * kQueryChunk + threadIdx.x;
        if (c < full) query_rows<NG, false>(state, ctrl, rows, base, q, nb, nr, sGoal, sCount, sFirst, sBest);
        else query_rows<NG, true>(state, ctrl, rows, base, q, nb, nr, sGoal, sCount, sFirst, sBest);
    }
    // nearest: lanes -> wave -> workgroup
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        unsigned long long key = ((unsigned long long)nb[g] << 32) | nr[g];   // kNoGoalKey for a lane without rows
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(key, off, 64);
            key = other < key ? other : key;
        }
        if ((threadIdx.x & 63) == 0 && key != kNoGoalKey) atomicMin(&sNear[g], key);
    }
    __syncthreads();
    // one global atomic per workgroup, goal and field that changed
    if ((int)threadIdx.x < n) {
        const int g = threadIdx.x;
        if (sCount[g]) {
            atomicAdd(&acc[g].count, sCount[g]);
            atomicMin(&acc[g].first, sFirst[g]);
            atomicMin(&acc[g].best, sBest[g]);
        }
        if (sNear[g] != kNoGoalKey) atomicMin(&acc[g].nearest, sNear[g]);
    }
}

// Workgroups of k_tree_query<NG> the device holds at once, at most kQueryGroupsPerCU per CU.
template <int NG>
int query_resident_groups() {
    static int cached[64] = {0};
    int dev = 0;
    SBMP_HIP(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && cached[dev]) return cached[dev];
    int perCU = 0, cus = 0;
    SBMP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, k_tree_query<NG>, kQueryBlock, 0));
    SBMP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (perCU < 1 || cus < 1) throw Error(SBMP_ERR_HIP, "k_tree_query: the occupancy query gave no resident workgroup");
    const int groups = std::min(perCU, kQueryGroupsPerCU) * cus;
    if (dev >= 0 && dev < 64) cached[dev] = groups;
    return groups;
}

// One pass for the goals [first, first + n) of xyt (n <= NG).
template <int NG>
void launch_query_tile(const float4* state, const float4* ctrl, long long rows, const float* xyt, int first, int n,
                       QueryAcc* acc, hipStream_t s) {
    QueryTile<NG> q;
    for (int g = 0; g < NG; ++g) {
        const bool real = g < n;
        q.gx[g] = real ? xyt[3 * (size_t)(first + g)] : 0.0f;
        q.gy[g] = real ? xyt[3 * (size_t)(first + g) + 1] : 0.0f;
        q.t[g] = real ? xyt[3 * (size_t)(first + g) + 2] : -1.0f;
    }
    const long long chunks = (rows + kQueryChunk - 1) / kQueryChunk;
    const int grid = (int)std::min<long long>(query_resident_groups<NG>(), chunks);
    hipLaunchKernelGGL(k_tree_query<NG>, dim3(grid), dim3(kQueryBlock), 0, s, state, ctrl, rows, q, n, acc + first);
}

void check_query_rows(const void* state, const void* ctrl, long long rows) {
    if (!state || !ctrl) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state and ctrl must be non-NULL");
    if (rows < 1 || rows > 0x7fffffffll) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
}

}  // namespace

sbmp_goal_answer goal_answer_of(unsigned count, unsigned first, unsigned long long best, unsigned long long nearest) {
    sbmp_goal_answer a;
    a.count = (int)count;
    a.firstRow = count ? (int)first : -1;
    a.bestRow = count ? (int)(uint32_t)best : -1;
    a.bestCost = count ? u2f((uint32_t)(best >> 32)) : 0.0f;
    a.nearestRow = (int)(uint32_t)nearest;
    a.nearestDistance = __builtin_sqrtf(u2f((uint32_t)(nearest >> 32)));
    return a;
}

void launch_tree_query(const float4* state, const float4* ctrl, long long rows, const float* goalsXYT, int count,
                       QueryAcc* acc, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_tree_query_init, dim3((count + 255) / 256), dim3(256), 0, s, acc, count);
    // whole tiles of kQueryTile goals, then the rest in the smallest tile that holds it
    for (int first = 0; first < count;) {
        const int left = count - first;
        if (left > 8) {
            launch_query_tile<kQueryTile>(state, ctrl, rows, goalsXYT, first, std::min(left, kQueryTile), acc, s);
        } else if (left > 4) {
            launch_query_tile<8>(state, ctrl, rows, goalsXYT, first, left, acc, s);
        } else if (left > 2) {
            launch_query_tile<4>(state, ctrl, rows, goalsXYT, first, left, acc, s);
        } else if (left > 1) {
            launch_query_tile<2>(state, ctrl, rows, goalsXYT, first, left, acc, s);
        } else {
            launch_query_tile<1>(state, ctrl, rows, goalsXYT, first, left, acc, s);
        }
        first += std::min(left, kQueryTile);
    }
    SBMP_HIP(hipGetLastError());
}

void tree_query_check_goals(const sbmp_goal_query* goals, int count, const sbmp_goal_answer* out) {
    if (count < 0) throw Error(SBMP_ERR_INVALID_ARGUMENT, "count must be >= 0");
    if (count > 0 && (!goals || !out)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "goals and out must be non-NULL");
    for (int i = 0; i < count; ++i)
        if (!std::isfinite(goals[i].x) || !std::isfinite(goals[i].y))
            throw Error(SBMP_ERR_INVALID_ARGUMENT, "goal " + std::to_string(i) + " has a non-finite coordinate");
}

// The goals' thresholds on the host, the kernel on `stream`, the keys back and into answers.
// Waits for the result.
void tree_query_device(const float* d_state, const float* d_ctrl, long long rows, const sbmp_goal_query* goals,
                       int count, sbmp_goal_answer* out, hipStream_t stream) {
    tree_query_check_goals(goals, count, out);
    check_query_rows(d_state, d_ctrl, rows);
    if (count == 0) return;
    std::vector<float> xyt(3 * (size_t)count);
    for (int i = 0; i < count; ++i) {
        xyt[3 * (size_t)i] = goals[i].x;
        xyt[3 * (size_t)i + 1] = goals[i].y;
        xyt[3 * (size_t)i + 2] = goal_radius_threshold(goals[i].radius);
    }
    std::vector<QueryAcc> host(count);
    QueryAcc* acc = nullptr;
    SBMP_HIP(hipMalloc(reinterpret_cast<void**>(&acc), sizeof(QueryAcc) * (size_t)count));
    hipError_t e = hipSuccess;
    try {
        launch_tree_query(reinterpret_cast<const float4*>(d_state), reinterpret_cast<const float4*>(d_ctrl), rows,
                          xyt.data(), count, acc, stream);
        e = hipMemcpyAsync(host.data(), acc, sizeof(QueryAcc) * (size_t)count, hipMemcpyDeviceToHost, stream);
        const hipError_t e2 = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = e2;
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(acc);
        throw;
    }
    (void)hipFree(acc);
    SBMP_HIP(e);
    for (int i = 0; i < count; ++i) out[i] = goal_answer_of(host[i].count, host[i].first, host[i].best, host[i].nearest);
}

// The literal rule, row by row (no threshold): what the kernel must reproduce.
void tree_query_host(const float* state, const float* ctrl, long long rows, const sbmp_goal_query* goals, int count,
                     sbmp_goal_answer* out) {
    tree_query_check_goals(goals, count, out);
    check_query_rows(state, ctrl, rows);
    for (int i = 0; i < count; ++i) {
        unsigned n = 0u, first = ~0u;
        unsigned long long best = kNoGoalKey, nearest = kNoGoalKey;
        for (long long row = 0; row < rows; ++row) {
            const float d2 = goal_d2(state[4 * row], state[4 * row + 1], goals[i].x, goals[i].y);
            const unsigned long long nk = goal_key(d2, (uint32_t)row);
            if (nk < nearest) nearest = nk;
            if (!goal_inside(d2, goals[i].radius)) continue;
            ++n;
            if ((unsigned)row < first) first = (unsigned)row;
            const unsigned long long bk = goal_key(ctrl[4 * row + 3], (uint32_t)row);
            if (bk < best) best = bk;
        }
        out[i] = goal_answer_of(n, first, best, nearest);
    }
}

}  // namespace sbmp

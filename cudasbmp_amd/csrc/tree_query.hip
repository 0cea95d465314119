// tree_query.hip — goal queries against a grown tree (include/sbmp/tree_query.h states the
// rule): for each goal disc, how many rows lie inside, the lowest of them,
// the cheapest of them, and the row nearest to the centre.
//   k_tree_query             one streaming pass over the rows for a tile of up to 16 goals
//   k_tree_query_alive       the same query over the rows a re-check (tree_recheck.hip) left
//                            alive: one masked row per lane, tiles of 8, 4 and 1
//   sbmp_tree_query_batch    the kernel over caller rows (tree_query_device)
//   sbmp_tree_query_batch_host   a plain host loop with the literal rule (tree_query_host)
//   sbmp_tree_query_alive_batch / _host   the masked kernel and the masked loop over caller rows
//   sbmp_kgmt_query_goals    the kernel over a planner's tree (KgmtPlanner::query_goals)
//   sbmp_kgmt_query_goals_alive  the masked kernel (KgmtPlanner::query_goals_alive)
// The kernels read treeState once, 16 B per row; a row's cost (treeCtrl.w) is read only by
// a lane whose row is inside some disc.  Every reduction is an integer add or an unsigned
// minimum (of a row, or of goal_key = value bits << 32 | row), so the answer does not
// depend on the order rows arrive in: it is the same bits on every run, whatever the grid.
// The two kernels share the tile, the init kernel and the host path (goal_query_device); the
// grid, the buffers and the read-back are tree_pass.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_query.h"
#include "tree_pass.h"

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
    float gx[NG], gy[NG], t[NG];   // t: goal_radius_threshold(radius); -1 for padding
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
    // nearest: lanes -> wave -> workgroup.  (k_tree_query_alive ends with a copy of these 20
    // lines, to be edited together: as one function that both kernels call, in four shapes, the
    // compiler moved k_tree_query<1>'s row loop, and in two of them every instantiation's.)
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

// The masked query: a row whose alive byte is 0 is skipped as if the tree did not hold it.
// A kernel of its own, shaped differently on purpose (one row per lane and sweep, no slack
// test: the mask already thins the rows), so that no k_tree_query instantiation changes.
template <int NG>
__global__ __launch_bounds__(kQueryBlock) void k_tree_query_alive(const float4* __restrict__ state,
                                                                  const float4* __restrict__ ctrl,
                                                                  const uint8_t* __restrict__ alive, long long rows,
                                                                  QueryTile<NG> q, int n, QueryAcc* __restrict__ acc) {
    __shared__ unsigned sCount[NG], sFirst[NG];
    __shared__ unsigned long long sBest[NG], sNear[NG];
    if (threadIdx.x < NG) {
        sCount[threadIdx.x] = 0u;
        sFirst[threadIdx.x] = ~0u;
        sBest[threadIdx.x] = kNoGoalKey;
        sNear[threadIdx.x] = kNoGoalKey;
    }
    __syncthreads();
    uint32_t nb[NG], nr[NG];   // the lane's lowest d2 (as bits: d2 >= 0) per goal and its row
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        nb[g] = ~0u;
        nr[g] = ~0u;
    }
    const long long stride = (long long)gridDim.x * kQueryBlock;
    for (long long row = (long long)blockIdx.x * kQueryBlock + threadIdx.x; row < rows; row += stride) {
        if (!alive[row]) continue;
        const float4 s = state[row];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float d2 = goal_d2(s.x, s.y, q.gx[g], q.gy[g]);
            const uint32_t b = __float_as_uint(d2);
            if (b < nb[g]) {   // a lane meets its rows in ascending order: the lowest row of equal d2 stays
                nb[g] = b;
                nr[g] = (uint32_t)row;
            }
            if (d2 <= q.t[g]) {
                atomicAdd(&sCount[g], 1u);
                atomicMin(&sFirst[g], (unsigned)row);
                atomicMin(&sBest[g], goal_key(ctrl[row].w, (uint32_t)row));
            }
        }
    }
    // k_tree_query's epilogue (see there)
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
// Cached per device: a single-tile query is short enough for the occupancy query to show.
template <int NG>
int query_resident_groups() {
    static int cached[64] = {0};
    int dev = 0;
    SBMP_HIP(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && cached[dev]) return cached[dev];
    const int groups = resident_grid(k_tree_query<NG>, kQueryBlock, 0, kQueryGroupsPerCU, kWholeDevice, "k_tree_query");
    if (dev >= 0 && dev < 64) cached[dev] = groups;
    return groups;
}

// The goals [first, first + n) of xyt (n <= NG) as a tile; the rest is padding.
template <int NG>
QueryTile<NG> fill_query_tile(const float* xyt, int first, int n) {
    QueryTile<NG> q;
    for (int g = 0; g < NG; ++g) {
        const bool real = g < n;
        q.gx[g] = real ? xyt[3 * (size_t)(first + g)] : 0.0f;
        q.gy[g] = real ? xyt[3 * (size_t)(first + g) + 1] : 0.0f;
        q.t[g] = real ? xyt[3 * (size_t)(first + g) + 2] : -1.0f;
    }
    return q;
}

// One pass for the goals [first, first + n) of xyt (n <= NG).
template <int NG>
void launch_query_tile(const float4* state, const float4* ctrl, long long rows, const float* xyt, int first, int n,
                       QueryAcc* acc, hipStream_t s) {
    const long long chunks = (rows + kQueryChunk - 1) / kQueryChunk;
    const int grid = (int)std::min<long long>(query_resident_groups<NG>(), chunks);
    hipLaunchKernelGGL(k_tree_query<NG>, dim3(grid), dim3(kQueryBlock), 0, s, state, ctrl, rows,
                       fill_query_tile<NG>(xyt, first, n), n, acc + first);
}

template <int NG>
void launch_alive_tile(const float4* state, const float4* ctrl, const uint8_t* alive, long long rows, const float* xyt,
                       int first, int n, QueryAcc* acc, hipStream_t s) {
    const int grid = resident_grid(k_tree_query_alive<NG>, kQueryBlock, 0, kQueryGroupsPerCU, rows, "k_tree_query_alive");
    hipLaunchKernelGGL(k_tree_query_alive<NG>, dim3(grid), dim3(kQueryBlock), 0, s, state, ctrl, alive, rows,
                       fill_query_tile<NG>(xyt, first, n), n, acc + first);
}

void launch_query_init(QueryAcc* acc, int count, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_query_init, dim3((count + 255) / 256), dim3(256), 0, s, acc, count);
}

// The masked query's launches: tiles of 8 (its centres and thresholds still fit the SGPRs), 4, 1.
void launch_tree_query_alive(const float4* state, const float4* ctrl, const uint8_t* alive, long long rows,
                             const float* xyt, int count, QueryAcc* acc, hipStream_t s) {
    launch_query_init(acc, count, s);
    for (int first = 0; first < count;) {
        const int left = count - first;
        const int n = left >= 8 ? 8 : left >= 4 ? 4 : 1;
        if (n == 8) launch_alive_tile<8>(state, ctrl, alive, rows, xyt, first, n, acc, s);
        else if (n == 4) launch_alive_tile<4>(state, ctrl, alive, rows, xyt, first, n, acc, s);
        else launch_alive_tile<1>(state, ctrl, alive, rows, xyt, first, n, acc, s);
        first += n;
    }
    SBMP_HIP(hipGetLastError());
}

void check_query_rows(long long rows) {
    if (rows < 1 || rows > 0x7fffffffll) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
}

// The host path of both queries: the goals' thresholds, the accumulators (the call's own), the
// launches (launch(xyt, acc): the init kernel and the tiles, on `stream`), the keys back and
// into answers.  Waits for the result.
template <class Launch>
void goal_query_device(const sbmp_goal_query* goals, int count, sbmp_goal_answer* out, hipStream_t stream,
                       Launch launch) {
    std::vector<float> xyt(3 * (size_t)count);
    for (int i = 0; i < count; ++i) {
        xyt[3 * (size_t)i] = goals[i].x;
        xyt[3 * (size_t)i + 1] = goals[i].y;
        xyt[3 * (size_t)i + 2] = goal_radius_threshold(goals[i].radius);
    }
    std::vector<QueryAcc> host(count);
    DevBufs w;
    QueryAcc* acc = w.alloc<QueryAcc>(count);
    drained_on_throw(stream, [&] {
        launch(xyt.data(), acc);
        read_back(stream, {{host.data(), acc, sizeof(QueryAcc) * (size_t)count}});
    });
    for (int i = 0; i < count; ++i) out[i] = goal_answer_of(host[i].count, host[i].first, host[i].best, host[i].nearest);
}

}  // namespace

void launch_tree_query(const float4* state, const float4* ctrl, long long rows, const float* goalsXYT, int count,
                       QueryAcc* acc, hipStream_t s) {
    if (count <= 0) return;
    launch_query_init(acc, count, s);
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

void tree_query_device(const float* d_state, const float* d_ctrl, long long rows, const sbmp_goal_query* goals,
                       int count, sbmp_goal_answer* out, hipStream_t stream) {
    tree_query_check_goals(goals, count, out);
    if (!d_state || !d_ctrl) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state and ctrl must be non-NULL");
    check_query_rows(rows);
    if (count == 0) return;
    goal_query_device(goals, count, out, stream, [&](const float* xyt, QueryAcc* acc) {
        launch_tree_query(reinterpret_cast<const float4*>(d_state), reinterpret_cast<const float4*>(d_ctrl), rows, xyt,
                          count, acc, stream);
    });
}

void tree_query_alive_device(const float* d_state, const float* d_ctrl, const uint8_t* d_alive, long long rows,
                             const sbmp_goal_query* goals, int count, sbmp_goal_answer* out, hipStream_t stream) {
    tree_query_check_goals(goals, count, out);
    if (!d_state || !d_ctrl || !d_alive) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and alive must be non-NULL");
    check_query_rows(rows);
    if (count == 0) return;
    goal_query_device(goals, count, out, stream, [&](const float* xyt, QueryAcc* acc) {
        launch_tree_query_alive(reinterpret_cast<const float4*>(d_state), reinterpret_cast<const float4*>(d_ctrl),
                                d_alive, rows, xyt, count, acc, stream);
    });
}

// The literal rule, row by row (query_rows_host, include/sbmp/tree_query.h).
void tree_query_host(const float* state, const float* ctrl, long long rows, const sbmp_goal_query* goals, int count,
                     sbmp_goal_answer* out) {
    tree_query_check_goals(goals, count, out);
    if (!state || !ctrl) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state and ctrl must be non-NULL");
    check_query_rows(rows);
    query_rows_host(state, ctrl, nullptr, rows, goals, count, out);
}

void tree_query_alive_host(const float* state, const float* ctrl, const uint8_t* alive, long long rows,
                           const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) {
    tree_query_check_goals(goals, count, out);
    if (!state || !ctrl || !alive) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and alive must be non-NULL");
    check_query_rows(rows);
    query_rows_host(state, ctrl, alive, rows, goals, count, out);
}

}  // namespace sbmp

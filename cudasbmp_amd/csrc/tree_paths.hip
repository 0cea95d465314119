// tree_paths.hip — the output stage of a grown tree (include/sbmp/tree_paths.h states the rule;
// DESIGN.md §5.10).
//   k_path_walk<EMIT>     one lane per request.  Pass A (EMIT = false) walks the parent chain and
//                         writes the request's length and status; the host sums the lengths (64-bit
//                         exclusive scan); pass B (EMIT = true) walks again and writes the rows, the
//                         7 sample floats and the cost of every path row at offset + length - 1 - k,
//                         root first.  Every loop is bounded by depthBound and a usable parent is a
//                         strictly lower row; no lane waits for another.
//   k_tree_trace<AGENT>   one lane per listed row (or per row of [0, count)): the row's parent
//                         first; behind the orphan test the parent's state, the row's controls and
//                         state (stored_controls); then car_trace / point_trace, the expand step's
//                         Euler updates (car_euler / point_euler of kgmt_device.h) without the cull,
//                         the predicates and the exec masking.  Every step is one 16-byte store per lane,
//                         step-major, consecutive lanes on consecutive addresses; one status byte.
//   sbmp_tree_paths_batch / _host, sbmp_tree_trace_batch / _host, and what
//   sbmp_kgmt_solution_paths / sbmp_kgmt_trace_rows run (KgmtPlanner::solution_paths, trace_rows)
// Stream order between the launches is the only ordering; every output element has one writer.
// The trace's grid, the buffers and the read-backs are tree_pass.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_paths.h"
#include "sbmp/tree_recheck.h"
#include "tree_pass.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

namespace {
constexpr int kPathsBlock = 256;        // lanes per workgroup
constexpr int kTraceGroupsPerCU = 8;    // as k_tree_query / k_tree_recheck: one sweep is at most CUs x 8 x 256 rows

template <bool EMIT>
__global__ __launch_bounds__(kPathsBlock) void k_path_walk(const float4* __restrict__ tState,
                                                           const float4* __restrict__ tCtrl,
                                                           const int* __restrict__ tParent, int depthBound,
                                                           const int* __restrict__ nodes, int count,
                                                           int* __restrict__ lengths, uint8_t* __restrict__ status,
                                                           const long long* __restrict__ offsets,
                                                           int* __restrict__ rows, float* __restrict__ samples,
                                                           float* __restrict__ costs) {
    const int i = blockIdx.x * kPathsBlock + threadIdx.x;
    if (i >= count) return;
    const int node = nodes[i];
    int len = 0;
    if (!EMIT) {
        const uint8_t st = path_walk(tParent, node, depthBound, &len, false, [](int, int) {});
        lengths[i] = len;
        status[i] = st;
    } else {
        const int mine = lengths[i];   // pass A's: > 0 only for SBMP_PATH_OK
        if (mine <= 0) return;
        const long long last = offsets[i] + mine - 1;
        path_walk(tParent, node, depthBound, &len, true, [&](int k, int row) {
            const size_t at = (size_t)(last - k);
            if (rows) rows[at] = row;
            const float4 c = tCtrl[row];
            if (samples) {
                const float4 s = tState[row];
                float* o = samples + 7 * at;
                o[0] = s.x; o[1] = s.y; o[2] = s.z; o[3] = s.w;
                o[4] = c.x; o[5] = c.y; o[6] = c.z;
            }
            if (costs) costs[at] = c.w;
        });
    }
}

// car_euler's state updates (kgmt_device.h) and nothing else: the same sincos_pred, the same
// v / L switch (one multiply for a power-of-two L, else div_by with the IEEE fallback), the same
// packed pair FMAs, so every step is the float the planner integrated.  A hand copy, to be
// edited with car_euler's step: sharing one function moved every car kernel's code (see
// point_step, kgmt_device.h).  out: the lane's first step; the next step lies `stride`
// float4s on.
__device__ __forceinline__ float4 car_trace(float4 p, const ChildCtl& ctl, const KgmtDev& d, float4* out, size_t stride) {
    const float a = ctl.a, dt = ctl.dt, tan_steering = ctl.tanS;
    sbmp_f32x2 xy = {p.x, p.y}, tv = {p.z, p.w};
    const sbmp_f32x2 dt2 = {dt, dt};
    auto step = [&](auto invL) {
        float st, ct;
        sincos_pred(tv.x, &st, &ct);
        const sbmp_f32x2 nxy = __builtin_elementwise_fma(sbmp_f32x2{tv.y, tv.y} * sbmp_f32x2{ct, st}, dt2, xy);
        const float v = tv.y;
        float vl;
        if (decltype(invL)::value) {
            vl = v * d.invAgentLength;
        } else {
            vl = div_by(v, d.agentLength, d.rcpAgentLength);
            const bool slow = (d.rcpAgentLength == 0.0f) | !(__builtin_fabsf(v) >= 0x1p-100f) |
                              !(__builtin_fabsf(v) <= 0x1p100f);
            if (__ballot(slow) != 0ull && slow) vl = v / d.agentLength;
        }
        const sbmp_f32x2 ntv = __builtin_elementwise_fma(sbmp_f32x2{vl * tan_steering, a}, dt2, tv);
        xy = nxy;
        tv = ntv;
        *out = make_float4(xy.x, xy.y, tv.x, tv.y);
        out += stride;
    };
    const int nSteps = __builtin_amdgcn_readfirstlane(d.numDisc);
    if (d.invAgentLength != 0.0f) {
        for (int i = 0; i < nSteps; ++i) step(std::true_type());
    } else {
        for (int i = 0; i < nSteps; ++i) step(std::false_type());
    }
    return make_float4(xy.x, xy.y, tv.x, tv.y);
}

// point_euler's loop likewise: point_step and a store.
__device__ __forceinline__ float4 point_trace(float4 p, const ChildCtl& ctl, const KgmtDev& d, float4* out, size_t stride) {
    float x = p.x, y = p.y;
    const int nSteps = __builtin_amdgcn_readfirstlane(d.numDisc);
    for (int i = 0; i < nSteps; ++i) {
        point_step(x, y, ctl.a, ctl.steer, ctl.dt, x, y);
        *out = make_float4(x, y, 0.0f, 0.0f);
        out += stride;
    }
    return make_float4(x, y, 0.0f, 0.0f);
}

// list: count rows of the tree, or null for the rows [0, count).  steps: numDisc x count float4s,
// step-major.  Every listed row was checked against the tree's rows before the launch.
template <int AGENT>
__global__ __launch_bounds__(kPathsBlock) void k_tree_trace(KgmtDev d, const int* __restrict__ list, unsigned count,
                                                            float4* __restrict__ steps, uint8_t* __restrict__ status) {
    // The row loop's pointers in vector registers, as k_tree_recheck holds them: as uniform values
    // they sit in SGPRs next to the plan's parameters across the Euler loop.
    const float4* tState = d.treeState;
    const float4* tCtrl = d.treeCtrl;
    const int* tParent = d.treeParent;
    asm volatile("" : "+v"(status), "+v"(steps), "+v"(tState), "+v"(tCtrl), "+v"(tParent));
    const size_t plane = count;   // float4s between two steps of one entry: 64-bit, count x numDisc x 16 passes 2^32
    // unsigned: count < 2^31 and a sweep is at most 2^19 entries, so i + stride cannot wrap
    const unsigned stride = gridDim.x * kPathsBlock;
    for (unsigned i = blockIdx.x * kPathsBlock + threadIdx.x; i < count; i += stride) {
        const int r = list ? list[i] : (int)i;
        const int parent = tParent[r];
        const float4 me = tState[r];
        float4* out = steps + i;
        uint8_t st;
        if (r == 0 || !recheck_parent_usable(parent, r)) {
            const int nSteps = __builtin_amdgcn_readfirstlane(d.numDisc);
            for (int j = 0; j < nSteps; ++j, out += plane) *out = me;
            st = r == 0 ? SBMP_ROW_FREE : SBMP_ROW_ORPHAN;
        } else {
            const float4 p = tState[parent];
            const ChildCtl ctl = stored_controls<AGENT>(tCtrl[r], d);
            const float4 e = (AGENT == 0) ? car_trace(p, ctl, d, out, plane) : point_trace(p, ctl, d, out, plane);
            st = recheck_same_state(e.x, e.y, e.z, e.w, me.x, me.y, me.z, me.w) ? SBMP_ROW_FREE : SBMP_ROW_STALE;
        }
        status[i] = st;
    }
}

void check_paths_args(const sbmp_tree_paths_args* a) {
    if (!a) throw Error(SBMP_ERR_INVALID_ARGUMENT, "args must be non-NULL");
    if (!a->state || !a->ctrl || !a->parent) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and parent must be non-NULL");
    if (a->rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
}

void check_trace_args(const sbmp_tree_paths_args* a) {
    check_paths_args(a);
    if (a->numDisc < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "numDisc must be >= 1");
    if (a->agent != SBMP_AGENT_CAR && a->agent != SBMP_AGENT_POINT) throw Error(SBMP_ERR_INVALID_ARGUMENT, "agent");
}

int bound_of(const sbmp_tree_paths_args* a) { return a->depthBound > 0 ? a->depthBound : a->rows; }

// what the kernels read of a plan
KgmtDev dev_of(const sbmp_tree_paths_args* a) {
    KgmtDev d{};
    set_euler_params(d, std::max(a->numDisc, 1), a->agentLength);
    d.treeState = reinterpret_cast<float4*>(const_cast<float*>(a->state));
    d.treeCtrl = reinterpret_cast<float4*>(const_cast<float*>(a->ctrl));
    d.treeParent = const_cast<int*>(a->parent);
    return d;
}
}  // namespace

void tree_paths_check(const int* nodes, int count, int rows, const long long* total) {
    if (!total) throw Error(SBMP_ERR_INVALID_ARGUMENT, "total must be non-NULL");
    if (count < 0 || (count > 0 && !nodes)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad node list");
    if (!path_nodes_valid(nodes, count, rows))
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "a node is neither -1 nor a row of [0, " + std::to_string(rows) + ")");
}

// The two passes of k_path_walk over device arrays, queued on `stream` (no wait): pass A writes
// d_len and d_status; pass B reads d_len and the 64-bit row offsets d_off and writes the rows,
// samples and costs that are non-null.  tree_resample.hip walks its paths through them too.
void path_walk_lengths_device(const KgmtDev& d, int depthBound, const int* d_nodes, int count, int* d_len,
                              uint8_t* d_status, hipStream_t stream) {
    const int grid = (count + kPathsBlock - 1) / kPathsBlock;
    hipLaunchKernelGGL(k_path_walk<false>, dim3(grid), dim3(kPathsBlock), 0, stream, (const float4*)d.treeState,
                       (const float4*)d.treeCtrl, (const int*)d.treeParent, depthBound, d_nodes, count, d_len, d_status,
                       (const long long*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr);
    SBMP_HIP(hipGetLastError());
}

void path_walk_rows_device(const KgmtDev& d, int depthBound, const int* d_nodes, int count, int* d_len,
                           uint8_t* d_status, const long long* d_off, int* d_rows, float* d_samples, float* d_costs,
                           hipStream_t stream) {
    const int grid = (count + kPathsBlock - 1) / kPathsBlock;
    hipLaunchKernelGGL(k_path_walk<true>, dim3(grid), dim3(kPathsBlock), 0, stream, (const float4*)d.treeState,
                       (const float4*)d.treeCtrl, (const int*)d.treeParent, depthBound, d_nodes, count, d_len, d_status,
                       d_off, d_rows, d_samples, d_costs);
    SBMP_HIP(hipGetLastError());
}

void tree_paths_device(const KgmtDev& d, int rows, int depthBound, const int* nodes, int count, int* lengths,
                       uint8_t* status, int* outRows, float* samples, float* costs, long long capacity,
                       long long* total, hipStream_t stream) {
    *total = 0;
    if (count == 0) return;
    (void)rows;
    DevBufs w;
    drained_on_throw(stream, [&] {
        int* dNodes = w.alloc<int>(count);
        int* dLen = w.alloc<int>(count);
        uint8_t* dStatus = w.alloc<uint8_t>(count);
        std::vector<int> hLen(count);
        SBMP_HIP(hipMemcpyAsync(dNodes, nodes, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, stream));
        path_walk_lengths_device(d, depthBound, dNodes, count, dLen, dStatus, stream);
        read_back(stream, {{hLen.data(), dLen, sizeof(int) * (size_t)count}, {status, dStatus, (size_t)count}});
        std::vector<long long> off(count);
        long long sum = 0;
        for (int i = 0; i < count; ++i) {
            off[i] = sum;
            sum += hLen[i];
        }
        *total = sum;
        if (lengths) std::copy(hLen.begin(), hLen.end(), lengths);
        if (!outRows && !samples && !costs) return;
        if (capacity < sum)
            throw Error(SBMP_ERR_INVALID_ARGUMENT,
                        "capacity " + std::to_string(capacity) + " < total path rows " + std::to_string(sum));
        if (sum == 0) return;
        long long* dOff = w.alloc<long long>(count);
        int* dRows = outRows ? w.alloc<int>((size_t)sum) : nullptr;
        float* dSamples = samples ? w.alloc<float>(7 * (size_t)sum) : nullptr;
        float* dCosts = costs ? w.alloc<float>((size_t)sum) : nullptr;
        SBMP_HIP(hipMemcpyAsync(dOff, off.data(), sizeof(long long) * (size_t)count, hipMemcpyHostToDevice, stream));
        path_walk_rows_device(d, depthBound, dNodes, count, dLen, dStatus, dOff, dRows, dSamples, dCosts, stream);
        read_back(stream, {{outRows, dRows, sizeof(int) * (size_t)sum},
                           {samples, dSamples, sizeof(float) * 7 * (size_t)sum},
                           {costs, dCosts, sizeof(float) * (size_t)sum}});
    });
}

void tree_trace_check(const int* list, long long count, int rows, const float* steps) {
    if (count < 1 || count > 0x7fffffffll) throw Error(SBMP_ERR_INVALID_ARGUMENT, "count must be in [0, 2^31)");
    if (!steps) throw Error(SBMP_ERR_INVALID_ARGUMENT, "steps must be non-NULL");
    if (!list) {
        if (count > rows)
            throw Error(SBMP_ERR_INVALID_ARGUMENT, "count " + std::to_string(count) + " > rows " + std::to_string(rows));
        return;
    }
    for (long long i = 0; i < count; ++i)
        if (list[i] < 0 || list[i] >= rows)
            throw Error(SBMP_ERR_INVALID_ARGUMENT, "row " + std::to_string(list[i]) + " is not in [0, " + std::to_string(rows) + ")");
}

void tree_trace_device(const KgmtDev& d, int agent, int rows, const int* d_list, long long count, float* d_steps,
                       uint8_t* d_status, hipStream_t stream) {
    (void)rows;
    using Fn = decltype(&k_tree_trace<0>);
    const Fn fn = (agent == SBMP_AGENT_POINT) ? k_tree_trace<1> : k_tree_trace<0>;
    const int grid = resident_grid(fn, kPathsBlock, 0, kTraceGroupsPerCU, count, "k_tree_trace");
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kPathsBlock), 0, stream, d, d_list, (unsigned)count,
                       reinterpret_cast<float4*>(d_steps), d_status);
    SBMP_HIP(hipGetLastError());
    SBMP_HIP(hipStreamSynchronize(stream));
}

void tree_trace_to_host(const KgmtDev& d, int agent, int rows, const int* list, long long count, float* steps,
                        uint8_t* status, hipStream_t stream) {
    DevBufs w;
    drained_on_throw(stream, [&] {
        const size_t floats = 4 * (size_t)d.numDisc * (size_t)count;
        int* dList = list ? w.alloc<int>((size_t)count) : nullptr;
        float* dSteps = w.alloc<float>(floats);
        uint8_t* dStatus = w.alloc<uint8_t>((size_t)count);
        if (list) SBMP_HIP(hipMemcpyAsync(dList, list, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, stream));
        tree_trace_device(d, agent, rows, dList, count, dSteps, dStatus, stream);
        read_back(stream, {{steps, dSteps, sizeof(float) * floats}, {status, dStatus, (size_t)count}});
    });
}

void tree_paths_batch(const sbmp_tree_paths_args* a, const int* nodes, int count, int* lengths, uint8_t* status,
                      int* rows, float* samples, float* costs, long long capacity, long long* total, hipStream_t stream) {
    if (total) *total = 0;
    check_paths_args(a);
    tree_paths_check(nodes, count, a->rows, total);
    tree_paths_device(dev_of(a), a->rows, bound_of(a), nodes, count, lengths, status, rows, samples, costs, capacity,
                      total, stream);
}

void tree_paths_batch_host(const sbmp_tree_paths_args* a, const int* nodes, int count, int* lengths, uint8_t* status,
                           int* rows, float* samples, float* costs, long long capacity, long long* total) {
    if (total) *total = 0;
    check_paths_args(a);
    tree_paths_check(nodes, count, a->rows, total);
    *total = path_rows_host(a->state, a->ctrl, a->parent, bound_of(a), nodes, count, lengths, status, false, nullptr,
                            nullptr, nullptr);
    if (!rows && !samples && !costs) return;
    if (capacity < *total)
        throw Error(SBMP_ERR_INVALID_ARGUMENT,
                    "capacity " + std::to_string(capacity) + " < total path rows " + std::to_string(*total));
    path_rows_host(a->state, a->ctrl, a->parent, bound_of(a), nodes, count, nullptr, nullptr, true, rows, samples, costs);
}

void tree_trace_batch(const sbmp_tree_paths_args* a, const int* d_rows, long long count, float* d_steps,
                      uint8_t* d_status, hipStream_t stream) {
    check_trace_args(a);
    if (count == 0) return;
    if (!d_status) throw Error(SBMP_ERR_INVALID_ARGUMENT, "status must be non-NULL");
    if (d_rows) {   // the list is read back: no row outside the tree reaches the kernel
        if (count < 1 || count > 0x7fffffffll) throw Error(SBMP_ERR_INVALID_ARGUMENT, "count must be in [0, 2^31)");
        std::vector<int> h((size_t)count);
        SBMP_HIP(hipMemcpyAsync(h.data(), d_rows, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, stream));
        SBMP_HIP(hipStreamSynchronize(stream));
        tree_trace_check(h.data(), count, a->rows, d_steps);
    } else {
        tree_trace_check(nullptr, count, a->rows, d_steps);
    }
    tree_trace_device(dev_of(a), a->agent, a->rows, d_rows, count, d_steps, d_status, stream);
}

void tree_trace_batch_host(const sbmp_tree_paths_args* a, const int* rows, long long count, float* steps,
                           uint8_t* status) {
    check_trace_args(a);
    if (count == 0) return;
    if (!status) throw Error(SBMP_ERR_INVALID_ARGUMENT, "status must be non-NULL");
    tree_trace_check(rows, count, a->rows, steps);
    trace_rows_host(a->state, a->ctrl, a->parent, a->agent, a->numDisc, a->agentLength, rows, count, steps, status);
}

}  // namespace sbmp

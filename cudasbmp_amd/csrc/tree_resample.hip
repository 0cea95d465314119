// tree_resample.hip — solution paths resampled at a fixed period (include/sbmp/tree_resample.h
// states the rule).
//   k_path_walk            passes A and B of tree_paths.hip as they are (path_walk_lengths_device,
//                          path_walk_rows_device): the lengths, the statuses and the path rows root
//                          first at 64-bit row offsets.
//   k_resample_clock       one lane per request: walks the request's rows forward, writes T_k as
//                          doubles beside the rows and n_i (-1: T / period >= 2^31 - 2).  The host
//                          reads the n_i back, sums them (64-bit, exclusive), checks the bound and
//                          the capacity, and allocates.
//   k_path_resample<AGENT> one lane per sample, grid-stride over 64-bit sample numbers.  A lane
//                          finds its request by bisecting the sample offsets and its edge by
//                          bisecting that path's T_k; loads the parent's state and the row's
//                          controls (stored_controls: the expand step's dt and tan(steering));
//                          takes j Euler steps of dt and one of alpha (car_resample, a hand copy of
//                          car_trace's step; point_step); stores one float4, one int, one double.
//                          Consecutive lanes write consecutive addresses.  The searches are bounded
//                          by log2, the Euler loop by numDisc; no lane waits for another; no
//                          atomics, no LDS, vector stores only.
// Every node is checked against the tree's rows on the host before anything is launched and a
// usable parent is a lower row >= 0, so every row k_path_walk writes is a row of the tree: the
// kernels form no address outside it.  Stream order between the launches is the only ordering;
// every output element has one writer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_paths.h"
#include "sbmp/tree_resample.h"
#include "tree_pass.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sbmp {

namespace {
constexpr int kResampleBlock = 256;      // lanes per workgroup
constexpr int kResampleGroupsPerCU = 8;  // as k_tree_trace: one sweep is at most CUs x 8 x 256 samples

// lengths[i] > 0 only for SBMP_PATH_OK (pass A); rows: pass B's, path i at offsets[i].
__global__ __launch_bounds__(kResampleBlock) void k_resample_clock(const float4* __restrict__ tCtrl,
                                                                   const int* __restrict__ lengths,
                                                                   const long long* __restrict__ offsets,
                                                                   const int* __restrict__ rows, int count,
                                                                   double period, double* __restrict__ T,
                                                                   int* __restrict__ n) {
    const int i = blockIdx.x * kResampleBlock + threadIdx.x;
    if (i >= count) return;
    const int L = lengths[i];
    if (L <= 0) {
        n[i] = 0;
        return;
    }
    const size_t base = (size_t)offsets[i];
    double t = 0.0;
    T[base] = t;
    for (int k = 1; k < L; ++k) {
        t = t + resample_edge_time(tCtrl[rows[base + k]].z);
        T[base + k] = t;
    }
    n[i] = resample_count(t, period);
}

// j steps of dt and one of alpha: car_trace's step (tree_paths.hip), itself car_euler's state
// updates (kgmt_device.h) and nothing else: the same sincos_pred, the same v / L switch, the same
// packed pair FMAs.  A hand copy, to be edited with them (see point_step, kgmt_device.h).
__device__ __forceinline__ float4 car_resample(float4 p, const ChildCtl& ctl, const KgmtDev& d, int j, float alpha) {
    const float a = ctl.a, tan_steering = ctl.tanS;
    sbmp_f32x2 xy = {p.x, p.y}, tv = {p.z, p.w};
    auto step = [&](auto invL, float h) {
        const sbmp_f32x2 h2 = {h, h};
        float st, ct;
        sincos_pred(tv.x, &st, &ct);
        const sbmp_f32x2 nxy = __builtin_elementwise_fma(sbmp_f32x2{tv.y, tv.y} * sbmp_f32x2{ct, st}, h2, xy);
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
        const sbmp_f32x2 ntv = __builtin_elementwise_fma(sbmp_f32x2{vl * tan_steering, a}, h2, tv);
        xy = nxy;
        tv = ntv;
    };
    if (d.invAgentLength != 0.0f) {
        for (int i = 0; i < j; ++i) step(std::true_type(), ctl.dt);
        step(std::true_type(), alpha);
    } else {
        for (int i = 0; i < j; ++i) step(std::false_type(), ctl.dt);
        step(std::false_type(), alpha);
    }
    return make_float4(xy.x, xy.y, tv.x, tv.y);
}

__device__ __forceinline__ float4 point_resample(float4 p, const ChildCtl& ctl, int j, float alpha) {
    float x = p.x, y = p.y;
    for (int i = 0; i < j; ++i) point_step(x, y, ctl.a, ctl.steer, ctl.dt, x, y);
    point_step(x, y, ctl.a, ctl.steer, alpha, x, y);
    return make_float4(x, y, 0.0f, 0.0f);
}

// sampleOff: count + 1 exclusive sums of the n_i, sampleOff[count] = total > 0.  rowOff, lengths,
// rows, T: the paths and their clocks.  Every row of `rows` is a row of the tree.
template <int AGENT>
__global__ __launch_bounds__(kResampleBlock) void k_path_resample(KgmtDev d, const long long* __restrict__ sampleOff,
                                                                  const long long* __restrict__ rowOff,
                                                                  const int* __restrict__ lengths,
                                                                  const int* __restrict__ rows,
                                                                  const double* __restrict__ T, int count,
                                                                  long long total, double period,
                                                                  float4* __restrict__ states, int* __restrict__ edges,
                                                                  double* __restrict__ times) {
    const float4* tState = d.treeState;
    const float4* tCtrl = d.treeCtrl;
    const long long stride = (long long)gridDim.x * kResampleBlock;
    for (long long s = (long long)blockIdx.x * kResampleBlock + threadIdx.x; s < total; s += stride) {
        // the last request whose offset is <= s: its n_i > 0, since the next offset is > s
        int lo = 0, hi = count - 1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo + 1) >> 1);
            if (sampleOff[mid] <= s) lo = mid;
            else hi = mid - 1;
        }
        const int i = lo;
        const long long first = sampleOff[i];
        const int m = (int)(s - first);
        const int n = (int)(sampleOff[i + 1] - first);
        const int L = lengths[i];
        const size_t base = (size_t)rowOff[i];
        const double* Ti = T + base;
        const double t = (double)m * period;
        const int k = (m == n - 1) ? L : resample_edge_of(Ti, L, t);
        float4 out;
        int edge;
        double time;
        if (k >= L) {
            edge = rows[base + L - 1];
            out = tState[edge];
            time = Ti[L - 1];
        } else {
            edge = rows[base + k];
            const float4 p = tState[rows[base + k - 1]];
            const ChildCtl ctl = stored_controls<AGENT>(tCtrl[edge], d);
            const double tau = t - Ti[k - 1];
            const int j = resample_step_of(tau, ctl.dt, d.numDisc);
            const float alpha = resample_alpha(tau, ctl.dt, j);
            out = (AGENT == 0) ? car_resample(p, ctl, d, j, alpha) : point_resample(p, ctl, j, alpha);
            time = t;
        }
        if (states) states[s] = out;
        if (edges) edges[s] = edge;
        if (times) times[s] = time;
    }
}

void check_resample_args(const sbmp_tree_paths_args* a) {
    if (!a) throw Error(SBMP_ERR_INVALID_ARGUMENT, "args must be non-NULL");
    if (!a->state || !a->ctrl || !a->parent) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and parent must be non-NULL");
    if (a->rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    if (a->numDisc < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "numDisc must be >= 1");
    if (a->agent != SBMP_AGENT_CAR && a->agent != SBMP_AGENT_POINT) throw Error(SBMP_ERR_INVALID_ARGUMENT, "agent");
}

int resample_bound_of(const sbmp_tree_paths_args* a) { return a->depthBound > 0 ? a->depthBound : a->rows; }

[[noreturn]] void throw_too_many() {
    throw Error(SBMP_ERR_INVALID_ARGUMENT, "a path's time / period is >= 2^31 - 2: too many samples");
}

void check_capacity(long long capacity, long long total) {
    if (capacity < total)
        throw Error(SBMP_ERR_INVALID_ARGUMENT,
                    "capacity " + std::to_string(capacity) + " < total samples " + std::to_string(total));
}
}  // namespace

void tree_resample_check(const int* nodes, int count, int rows, double period, const long long* total) {
    if (!total) throw Error(SBMP_ERR_INVALID_ARGUMENT, "total must be non-NULL");
    if (count < 0 || (count > 0 && !nodes)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad node list");
    if (!resample_period_valid(period)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "period must be finite and > 0");
    if (!path_nodes_valid(nodes, count, rows))
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "a node is neither -1 nor a row of [0, " + std::to_string(rows) + ")");
}

void tree_resample_device(const KgmtDev& d, int agent, int rows, int depthBound, const int* nodes, int count,
                          double period, int* counts, uint8_t* status, float* states, int* edges, double* times,
                          bool deviceOut, long long capacity, long long* total, hipStream_t stream) {
    *total = 0;
    if (count == 0) return;
    (void)rows;
    DevBufs w;
    drained_on_throw(stream, [&] {
        int* dNodes = w.alloc<int>(count);
        int* dLen = w.alloc<int>(count);
        uint8_t* dStatus = w.alloc<uint8_t>(count);
        std::vector<int> hLen(count), hN(count, 0);
        SBMP_HIP(hipMemcpyAsync(dNodes, nodes, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, stream));
        path_walk_lengths_device(d, depthBound, dNodes, count, dLen, dStatus, stream);
        read_back(stream, {{hLen.data(), dLen, sizeof(int) * (size_t)count}, {status, dStatus, (size_t)count}});
        std::vector<long long> rowOff(count);
        long long pathRows = 0;
        for (int i = 0; i < count; ++i) {
            rowOff[i] = pathRows;
            pathRows += hLen[i];
        }
        long long* dRowOff = nullptr;
        int* dRows = nullptr;
        double* dT = nullptr;
        if (pathRows > 0) {
            dRowOff = w.alloc<long long>(count);
            dRows = w.alloc<int>((size_t)pathRows);
            dT = w.alloc<double>((size_t)pathRows);
            int* dN = w.alloc<int>(count);
            SBMP_HIP(hipMemcpyAsync(dRowOff, rowOff.data(), sizeof(long long) * (size_t)count, hipMemcpyHostToDevice, stream));
            path_walk_rows_device(d, depthBound, dNodes, count, dLen, dStatus, dRowOff, dRows, nullptr, nullptr, stream);
            const int grid = (count + kResampleBlock - 1) / kResampleBlock;
            hipLaunchKernelGGL(k_resample_clock, dim3(grid), dim3(kResampleBlock), 0, stream, (const float4*)d.treeCtrl,
                               (const int*)dLen, (const long long*)dRowOff, (const int*)dRows, count, period, dT, dN);
            SBMP_HIP(hipGetLastError());
            read_back(stream, {{hN.data(), dN, sizeof(int) * (size_t)count}});
        }
        std::vector<long long> sampleOff((size_t)count + 1);
        long long sum = 0;
        for (int i = 0; i < count; ++i) {
            if (hN[i] < 0) throw_too_many();
            sampleOff[i] = sum;
            sum += hN[i];
        }
        sampleOff[count] = sum;
        *total = sum;
        if (counts) std::copy(hN.begin(), hN.end(), counts);
        if (!states && !edges && !times) return;
        check_capacity(capacity, sum);
        if (sum == 0) return;
        long long* dSampleOff = w.alloc<long long>((size_t)count + 1);
        SBMP_HIP(hipMemcpyAsync(dSampleOff, sampleOff.data(), sizeof(long long) * ((size_t)count + 1),
                                hipMemcpyHostToDevice, stream));
        float* dStates = states;
        int* dEdges = edges;
        double* dTimes = times;
        if (!deviceOut) {
            dStates = states ? w.alloc<float>(4 * (size_t)sum) : nullptr;
            dEdges = edges ? w.alloc<int>((size_t)sum) : nullptr;
            dTimes = times ? w.alloc<double>((size_t)sum) : nullptr;
        }
        using Fn = decltype(&k_path_resample<0>);
        const Fn fn = (agent == SBMP_AGENT_POINT) ? k_path_resample<1> : k_path_resample<0>;
        const int grid = resident_grid(fn, kResampleBlock, 0, kResampleGroupsPerCU, sum, "k_path_resample");
        hipLaunchKernelGGL(fn, dim3(grid), dim3(kResampleBlock), 0, stream, d, (const long long*)dSampleOff,
                           (const long long*)dRowOff, (const int*)dLen, (const int*)dRows, (const double*)dT, count, sum,
                           period, reinterpret_cast<float4*>(dStates), dEdges, dTimes);
        SBMP_HIP(hipGetLastError());
        if (deviceOut) {
            SBMP_HIP(hipStreamSynchronize(stream));
        } else {
            read_back(stream, {{states, dStates, sizeof(float) * 4 * (size_t)sum},
                               {edges, dEdges, sizeof(int) * (size_t)sum},
                               {times, dTimes, sizeof(double) * (size_t)sum}});
        }
    });
}

void tree_resample_batch(const sbmp_tree_paths_args* a, const int* nodes, int count, double period, int* counts,
                         uint8_t* status, float* d_states, int* d_edges, double* d_times, long long capacity,
                         long long* total, hipStream_t stream) {
    if (total) *total = 0;
    check_resample_args(a);
    tree_resample_check(nodes, count, a->rows, period, total);
    KgmtDev d{};
    set_euler_params(d, a->numDisc, a->agentLength);
    d.treeState = reinterpret_cast<float4*>(const_cast<float*>(a->state));
    d.treeCtrl = reinterpret_cast<float4*>(const_cast<float*>(a->ctrl));
    d.treeParent = const_cast<int*>(a->parent);
    tree_resample_device(d, a->agent, a->rows, resample_bound_of(a), nodes, count, period, counts, status, d_states,
                         d_edges, d_times, true, capacity, total, stream);
}

void tree_resample_batch_host(const sbmp_tree_paths_args* a, const int* nodes, int count, double period, int* counts,
                              uint8_t* status, float* states, int* edges, double* times, long long capacity,
                              long long* total) {
    if (total) *total = 0;
    check_resample_args(a);
    tree_resample_check(nodes, count, a->rows, period, total);
    const long long sum = resample_paths_host(a->state, a->ctrl, a->parent, resample_bound_of(a), a->agent, a->numDisc,
                                              a->agentLength, nodes, count, period, counts, status, false, nullptr,
                                              nullptr, nullptr);
    if (sum < 0) throw_too_many();
    *total = sum;
    if (!states && !edges && !times) return;
    check_capacity(capacity, sum);
    resample_paths_host(a->state, a->ctrl, a->parent, resample_bound_of(a), a->agent, a->numDisc, a->agentLength, nodes,
                        count, period, nullptr, nullptr, true, states, edges, times);
}

}  // namespace sbmp

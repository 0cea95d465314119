// tree_pass.h — the host-side plumbing of a pass over a grown tree, stated once for
// tree_query.hip, tree_recheck.hip, tree_paths.hip, tree_resample.hip, tree_extract.hip and
// tree_reanchor.hip (DESIGN.md §5.8–5.10, §5.12, §5.13, §5.15).  What a new tree pass gets for free:
//   resident_grid            the grid of a grid-stride kernel: what the device holds at once,
//                            no more than the work needs, and the one error when nothing fits
//   DevBufs                  the device buffers of one call, freed with it
//   drained_on_throw         a body whose exception leaves nothing in flight on the stream
//                            when those buffers go
//   read_back                results to the host: the copies, the wait, the first error
//   set_euler_params         what car_euler / point_euler (and their traces) read of a plan
//   attach_list              another obstacle list for those loops: its device copy, NaN scan
//                            and grid index, by begin()'s rule for the form
//   expand_variant_from_env  SBMP_EXPAND_VARIANT, as the planner reads it
// and on the device (kgmt_device.h): stored_controls, a row's controls as the ChildCtl the
// Euler loops take, and car_step / point_step, one Euler update of the state.
// KgmtPlanner::settled_rows (kgmt_planner.cpp) gives a planner's method the rows to pass over.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "obstacle_grid.h"

namespace sbmp {

// items: more than any device holds at once (the grid is then the resident workgroups alone)
constexpr long long kWholeDevice = 1ll << 40;

// Workgroups of `block` lanes for `items` lanes' worth of work: what the device holds at once
// of fn (at most groupsPerCU per CU, the occupancy query may give fewer), and no more than the
// items need.  Not cached: the query depends on fn, block and lds.
template <class Kernel>
int resident_grid(Kernel* fn, int block, size_t lds, int groupsPerCU, long long items, const char* name) {
    int dev = 0, perCU = 0, cus = 0;
    SBMP_HIP(hipGetDevice(&dev));
    SBMP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, reinterpret_cast<const void*>(fn), block, lds));
    SBMP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (perCU < 1 || cus < 1)
        throw Error(SBMP_ERR_HIP, std::string(name) + ": the occupancy query gave no resident workgroup");
    const long long need = (items + block - 1) / block;
    return (int)std::min<long long>((long long)std::min(perCU, groupsPerCU) * cus, std::max(need, 1ll));
}

// Device buffers of one call, freed with it.
struct DevBufs {
    std::vector<void*> p;
    DevBufs() = default;
    DevBufs(const DevBufs&) = delete;
    DevBufs& operator=(const DevBufs&) = delete;
    ~DevBufs() {
        for (void* q : p) (void)hipFree(q);
    }
    template <typename T>
    T* alloc(size_t n) {
        void* q = nullptr;
        SBMP_HIP(hipMalloc(&q, sizeof(T) * std::max<size_t>(n, 1)));
        p.push_back(q);
        return static_cast<T*>(q);
    }
};

// body(), and if it throws, the stream drained before the exception goes on: nothing is in
// flight when the call's DevBufs (declared before this) are freed.
template <class Body>
void drained_on_throw(hipStream_t stream, Body body) {
    try {
        body();
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        throw;
    }
}

// One copy of read_back; dst null: skipped.
struct HostCopy {
    void* dst;
    const void* src;
    size_t bytes;
};

// Queues the copies to the host on `stream`, waits for the stream, and throws the first error
// of either (the wait happens whatever the copies returned).
inline void read_back(hipStream_t stream, std::initializer_list<HostCopy> copies) {
    hipError_t e = hipSuccess;
    for (const HostCopy& c : copies)
        if (c.dst && e == hipSuccess) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = e2;
    SBMP_HIP(e);
}

// What the Euler loops read of a plan: numDisc, agentLength and their reciprocals.
// invAgentLength is set only for a power of two (then v * (1 / L) == v / L bitwise), else 0;
// rcpNumDisc / rcpAgentLength are div_by's verified reciprocals, or 0.
inline void set_euler_params(KgmtDev& d, int numDisc, float agentLength) {
    d.numDisc = numDisc;
    d.agentLength = agentLength;
    int e = 0;
    d.invAgentLength = (std::frexp(agentLength, &e) == 0.5f) ? 1.0f / agentLength : 0.0f;
    d.rcpNumDisc = markstein_rcp((float)numDisc);
    d.rcpAgentLength = markstein_rcp(agentLength);
}

// The new list's own device copy (in w: freed with the call), NaN scan and grid index, into d:
// a copy of the plan's parameters and tree pointers whose obstacle fields are replaced.
// The form follows begin()'s rule: the grid above kMaxLdsObs boxes (or variant 4), the
// global loop only for variant 5.
inline void attach_list(DevBufs& w, KgmtDev& d, const float* d_obstacles, int nObs, int variant, hipStream_t s) {
    d.obstacles = nullptr;
    d.nObs = nObs;
    d.obsNaN = 0;
    d.gridG = 0;
    d.gridInvW = d.gridInvH = 0.0f;
    d.gridStart = nullptr;
    d.gridBoxes = nullptr;
    if (nObs == 0) return;
    float4* obs = w.alloc<float4>((size_t)nObs);
    SBMP_HIP(hipMemcpyAsync(obs, d_obstacles, sizeof(float4) * (size_t)nObs, hipMemcpyDeviceToDevice, s));
    std::vector<float> h((size_t)4 * nObs);
    SBMP_HIP(hipMemcpyAsync(h.data(), d_obstacles, sizeof(float) * h.size(), hipMemcpyDeviceToHost, s));
    SBMP_HIP(hipStreamSynchronize(s));
    d.obstacles = obs;
    for (float v : h)   // wave_cull's and grid_free_fast's separation metric need boxes without NaN
        if (std::isnan(v)) d.obsNaN = 1;
    if (!((nObs > kMaxLdsObs && variant != 5) || variant == 4)) return;
    const HostObstacleGrid g =
        build_obstacle_grid(h.data(), nObs, d.width, d.height, std::min(grid_resolution(nObs), kMaxLdsGridG));
    // kGridBatch never-met rows past the end: grid_free_fast loads and tests whole batches
    const size_t nStart = g.start.size(), nBoxes = g.boxes.size() + kGridBatch;
    std::vector<float4> boxes(nBoxes, make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY));
    if (!g.boxes.empty()) std::memcpy(boxes.data(), g.boxes.data(), sizeof(float4) * g.boxes.size());
    int* gridStart = w.alloc<int>(nStart);
    float4* gridBoxes = w.alloc<float4>(nBoxes);
    SBMP_HIP(hipMemcpy(gridStart, g.start.data(), sizeof(int) * nStart, hipMemcpyHostToDevice));
    SBMP_HIP(hipMemcpy(gridBoxes, boxes.data(), sizeof(float4) * nBoxes, hipMemcpyHostToDevice));
    d.gridG = g.g;
    d.gridInvW = g.invW;
    d.gridInvH = g.invH;
    d.gridStart = gridStart;
    d.gridBoxes = gridBoxes;
}

// Obstacle-list form of the Euler loops (diagnostics / A-B): 0 auto, 1 LDS, 2 LDS x4,
// 3 registers, 4 grid index at any count, 5 global list without the grid.
inline int expand_variant_from_env() {
    const char* v = getenv("SBMP_EXPAND_VARIANT");
    return v ? std::min(5, std::max(0, atoi(v))) : 0;
}

}  // namespace sbmp

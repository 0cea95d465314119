// tree_extract.hip — the usable subtree of a grown tree as a tree of its own: prune and re-root
// (include/sbmp/tree_extract.h states the rule).
//   k_extract_mark     one lane per row: the first (anc, dead) pair.  dead: a row below the root,
//                      a masked row, a row above the root without a usable parent; anc = r for
//                      those, the root and the rows below it, else parent[r].  k_tree_alive's
//                      input convention with another initial condition
//   k_extract_jump     one pointer-jumping pass over double buffers: dead'[r] = dead[r] |
//                      dead[anc[r]], anc'[r] = anc[anc[r]] (§5.9's rule and sufficiency argument)
//   k_extract_count    the last pass: the member byte of every row, one member count per tile
//                      (the kExtractTileRows rows one workgroup numbers in one go) and the
//                      summary's four counters
//   k_extract_offsets  one workgroup: the exclusive sum of the tile counts, kExtractBlock tiles
//                      per round, and `kept`
//   k_extract_number   newRow of every row: the tile's offset, the wave totals before the lane's
//                      wave (LDS) and the members before the lane in its wave (ballot, popcount)
//   k_extract_gather   one lane per row: a member's two float4s, its origin and its remapped
//                      parent.  A launch after k_extract_number: newRow[parent[r]] may lie in
//                      any tile, and stream order between launches is the only ordering
//   sbmp_tree_extract_batch / _host, sbmp_tree_extract_info, sbmp_kgmt_extract_tree
// No lane or workgroup waits for another inside a kernel.  Every decision is an integer one and
// the summary is integer adds, so the bytes and the counts do not depend on the grid or on the
// order rows arrive in.  Row indices are 32-bit; every byte offset (16 x row) is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_extract.h"
#include "tree_pass.h"

namespace sbmp {

namespace {
constexpr int kExtractBlock = 256;      // lanes per workgroup
constexpr int kExtractWaves = kExtractBlock / 64;
constexpr int kExtractLaneRows = 4;     // rows of a tile per lane: row = tile base + j * 256 + lane
constexpr int kExtractTileRows = kExtractBlock * kExtractLaneRows;
constexpr int kExtractRoundTiles = kExtractBlock;   // tiles per round of k_extract_offsets, one per lane
constexpr int kExtractGroupsPerCU = 8;  // as the re-check's streaming passes

// The summary's accumulators (device): integer adds.
struct ExtractAcc {
    unsigned kept, below, masked, detached;
};

__global__ __launch_bounds__(kExtractBlock) void k_extract_mark(const int* __restrict__ parent,
                                                                const uint8_t* __restrict__ keep, int rows, int root,
                                                                int* __restrict__ anc0, uint8_t* __restrict__ dead0) {
    const long long stride = (long long)gridDim.x * kExtractBlock;
    for (long long row = (long long)blockIdx.x * kExtractBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const bool kept = extract_row_kept(keep, r);
        const int p = extract_reads_parent(r, root, kept) ? parent[r] : -1;
        const bool dead = extract_mark_dead(r, root, kept, p);
        anc0[r] = extract_mark_anc(r, root, dead, p);
        dead0[r] = dead ? 1 : 0;
    }
}

// deadIn[r] != 0 iff some row of r's chain covered so far cannot be a member.  ancIn[r] is a
// row of [0, r] by construction (k_extract_mark, and jumps only go up).
__global__ __launch_bounds__(kExtractBlock) void k_extract_jump(const int* __restrict__ ancIn, const uint8_t* deadIn,
                                                                int* __restrict__ ancOut, uint8_t* __restrict__ deadOut,
                                                                int rows) {
    const long long stride = (long long)gridDim.x * kExtractBlock;
    for (long long row = (long long)blockIdx.x * kExtractBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const int a = ancIn[r];
        deadOut[r] = deadIn[r] | deadIn[a];
        ancOut[r] = ancIn[a];
    }
}

// The last jump: member[r] = the whole chain of r is clear, the members of every tile, and the
// classes.  A workgroup takes whole tiles, so a tile's count has one writer.
__global__ __launch_bounds__(kExtractBlock) void k_extract_count(const int* __restrict__ ancIn, const uint8_t* deadIn,
                                                                 const uint8_t* __restrict__ keep, int rows, int root,
                                                                 int tiles, uint8_t* __restrict__ member,
                                                                 int* __restrict__ tileCount,
                                                                 ExtractAcc* __restrict__ acc) {
    __shared__ unsigned sAcc[4];
    __shared__ int sWave[kExtractWaves];
    if (threadIdx.x < 4) sAcc[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned n[4] = {0u, 0u, 0u, 0u};   // indexed by the class
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int waveMembers = 0;
#pragma unroll
        for (int j = 0; j < kExtractLaneRows; ++j) {
            const long long row = (long long)tile * kExtractTileRows + j * kExtractBlock + threadIdx.x;
            bool m = false;
            if (row < rows) {
                const int r = (int)row;
                const int a = ancIn[r];
                m = (deadIn[r] | deadIn[a]) == 0;
                member[r] = m ? 1 : 0;
                const int c = extract_row_class(r, root, extract_row_kept(keep, r), m);
                n[kExtractKept] += c == kExtractKept;
                n[kExtractBelow] += c == kExtractBelow;
                n[kExtractMasked] += c == kExtractMasked;
                n[kExtractDetached] += c == kExtractDetached;
            }
            waveMembers += (int)__popcll(__ballot(m));
        }
        if (lane == 0) sWave[wave] = waveMembers;
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = 0;
#pragma unroll
            for (int i = 0; i < kExtractWaves; ++i) sum += sWave[i];
            tileCount[tile] = sum;
        }
        __syncthreads();   // sWave is written again for the next tile
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (n[i]) atomicAdd(&sAcc[i], n[i]);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sAcc[kExtractKept]) atomicAdd(&acc->kept, sAcc[kExtractKept]);
        if (sAcc[kExtractBelow]) atomicAdd(&acc->below, sAcc[kExtractBelow]);
        if (sAcc[kExtractMasked]) atomicAdd(&acc->masked, sAcc[kExtractMasked]);
        if (sAcc[kExtractDetached]) atomicAdd(&acc->detached, sAcc[kExtractDetached]);
    }
}

// One workgroup: tileOff[t] = the members of the tiles before t; *kept = all of them.  A round
// takes kExtractRoundTiles tiles, one per lane; `base` carries the rounds before in a register.
__global__ __launch_bounds__(kExtractBlock) void k_extract_offsets(const int* __restrict__ tileCount, int tiles,
                                                                   int* __restrict__ tileOff, int* __restrict__ kept) {
    __shared__ int sWave[kExtractWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int t0 = 0; t0 < tiles; t0 += kExtractRoundTiles) {   // uniform: every lane is active in wave_incl_sum
        const int t = t0 + (int)threadIdx.x;
        const int c = t < tiles ? tileCount[t] : 0;
        const int incl = wave_incl_sum(c);
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kExtractWaves; ++i) {
            const int v = sWave[i];
            before += i < wave ? v : 0;
            total += v;
        }
        if (t < tiles) tileOff[t] = base + before + incl - c;
        base += total;
        __syncthreads();   // sWave is written again in the next round
    }
    if (threadIdx.x == 0) *kept = base;
}

// newRow of every row of the workgroup's tiles.  The order inside a tile is the row order:
// part j, then wave, then lane.
__global__ __launch_bounds__(kExtractBlock) void k_extract_number(const uint8_t* __restrict__ member, int rows,
                                                                  int tiles, const int* __restrict__ tileOff,
                                                                  int* __restrict__ newRow) {
    __shared__ int sWave[kExtractLaneRows * kExtractWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long first = (long long)tile * kExtractTileRows + threadIdx.x;
        bool m[kExtractLaneRows];
        int rank[kExtractLaneRows];   // members before the lane in its wave
#pragma unroll
        for (int j = 0; j < kExtractLaneRows; ++j) {
            const long long row = first + j * kExtractBlock;
            m[j] = row < rows && member[row] != 0;
            const unsigned long long b = __ballot(m[j]);
            rank[j] = (int)__popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) sWave[j * kExtractWaves + wave] = (int)__popcll(b);
        }
        __syncthreads();
        int run = tileOff[tile];
#pragma unroll
        for (int i = 0; i < kExtractLaneRows * kExtractWaves; ++i) {
            if ((i % kExtractWaves) == wave) {
                const int j = i / kExtractWaves;
                const long long row = first + j * kExtractBlock;
                if (row < rows) newRow[row] = m[j] ? run + rank[j] : -1;
            }
            run += sWave[i];
        }
        __syncthreads();   // sWave is written again for the next tile
    }
}

// A member's rows.  newRow[r] < kept <= the outputs' rows (checked by the host); a member above
// the root has a usable parent that is a member, so newRow[parent[r]] is a row of [0, newRow[r]).
__global__ __launch_bounds__(kExtractBlock) void k_extract_gather(const float4* __restrict__ tState,
                                                                  const float4* __restrict__ tCtrl,
                                                                  const int* __restrict__ tParent,
                                                                  const int* __restrict__ newRow, int rows, int root,
                                                                  float4* __restrict__ oState, float4* __restrict__ oCtrl,
                                                                  int* __restrict__ oParent, int* __restrict__ oOrigin) {
    const long long stride = (long long)gridDim.x * kExtractBlock;
    for (long long row = (long long)blockIdx.x * kExtractBlock + threadIdx.x; row < rows; row += stride) {
        const int r = (int)row;
        const long long k = newRow[r];
        if (k < 0) continue;
        if (oState) oState[k] = tState[row];
        if (oCtrl) oCtrl[k] = tCtrl[row];
        if (oOrigin) oOrigin[k] = r;
        if (oParent) oParent[k] = extract_new_parent(r, root, tParent, newRow);
    }
}

// ---------------------------------------------------------------- host side
template <class Kernel>
int extract_grid(Kernel* fn, long long lanes, const char* name) {
    return resident_grid(fn, kExtractBlock, 0, kExtractGroupsPerCU, lanes, name);
}

// ceil(log2(bound)): after that many passes dead[r] covers 2^passes >= bound rows of r's chain.
int extract_jump_passes(long long bound) {
    int p = 0;
    while ((1ll << p) < bound) ++p;
    return p;
}

int extract_tiles(long long rows) { return (int)((rows + kExtractTileRows - 1) / kExtractTileRows); }

void check_extract_capacity(long long capacity, int kept) {
    if (capacity < kept)
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " < kept rows " + std::to_string(kept));
}

void check_extract_args(const sbmp_tree_extract_args* a, int root, const sbmp_tree_extract* out) {
    if (!a || !out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "args and out must be non-NULL");
    if (!a->state || !a->ctrl || !a->parent) throw Error(SBMP_ERR_INVALID_ARGUMENT, "state, ctrl and parent must be non-NULL");
    if (a->rows < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [1, 2^31)");
    tree_extract_check_root(root, a->rows);
}
}  // namespace

void tree_extract_check_root(int root, int rows) {
    if (root < 0 || root >= rows)
        throw Error(SBMP_ERR_INVALID_ARGUMENT, "root " + std::to_string(root) + " is no row of [0, " + std::to_string(rows) + ")");
}

void tree_extract_device(const KgmtDev& d, int rows, int depthBound, int root, const uint8_t* d_keep, float* state,
                         float* ctrl, int* parent, int* origin, int* newRow, bool deviceOut, long long capacity,
                         sbmp_tree_extract* out, hipStream_t stream) {
    *out = sbmp_tree_extract{rows, 0, 0, 0, 0, root, 0.0f};
    const float4* tState = d.treeState;
    const float4* tCtrl = d.treeCtrl;
    const int* tParent = d.treeParent;
    DevBufs w;
    drained_on_throw(stream, [&] {
        const int passes = std::max(1, extract_jump_passes(depthBound > 0 ? std::min(depthBound, rows) : rows));
        const int tiles = extract_tiles(rows);
        const bool wantMembers = state || ctrl || parent || origin;
        int* anc[2] = {w.alloc<int>((size_t)rows), passes > 1 ? w.alloc<int>((size_t)rows) : nullptr};
        uint8_t* dead[2] = {w.alloc<uint8_t>((size_t)rows), passes > 1 ? w.alloc<uint8_t>((size_t)rows) : nullptr};
        uint8_t* member = w.alloc<uint8_t>((size_t)rows);
        int* tileCount = w.alloc<int>((size_t)tiles);
        int* tileOff = w.alloc<int>((size_t)tiles);
        int* dKept = w.alloc<int>(1);
        ExtractAcc* dAcc = w.alloc<ExtractAcc>(1);
        int* dNewRow = (deviceOut && newRow) ? newRow : (wantMembers || newRow) ? w.alloc<int>((size_t)rows) : nullptr;
        SBMP_HIP(hipMemsetAsync(dAcc, 0, sizeof(ExtractAcc), stream));

        const int gridRows = extract_grid(k_extract_mark, rows, "k_extract_mark");
        hipLaunchKernelGGL(k_extract_mark, dim3(gridRows), dim3(kExtractBlock), 0, stream, tParent, d_keep, rows, root,
                           anc[0], dead[0]);
        // pass p reads pair p & 1 and writes pair (p + 1) & 1; the last pass is k_extract_count
        const int gridJump = extract_grid(k_extract_jump, rows, "k_extract_jump");
        for (int p = 0; p + 1 < passes; ++p)
            hipLaunchKernelGGL(k_extract_jump, dim3(gridJump), dim3(kExtractBlock), 0, stream, (const int*)anc[p & 1],
                               (const uint8_t*)dead[p & 1], anc[(p + 1) & 1], dead[(p + 1) & 1], rows);
        const int last = passes - 1;
        const long long tileLanes = (long long)tiles * kExtractBlock;
        hipLaunchKernelGGL(k_extract_count, dim3(extract_grid(k_extract_count, tileLanes, "k_extract_count")),
                           dim3(kExtractBlock), 0, stream, (const int*)anc[last & 1], (const uint8_t*)dead[last & 1],
                           d_keep, rows, root, tiles, member, tileCount, dAcc);
        hipLaunchKernelGGL(k_extract_offsets, dim3(1), dim3(kExtractBlock), 0, stream, (const int*)tileCount, tiles,
                           tileOff, dKept);
        if (dNewRow)
            hipLaunchKernelGGL(k_extract_number, dim3(extract_grid(k_extract_number, tileLanes, "k_extract_number")),
                               dim3(kExtractBlock), 0, stream, (const uint8_t*)member, rows, tiles, (const int*)tileOff,
                               dNewRow);
        SBMP_HIP(hipGetLastError());
        // the host reads `kept` before the gather: the capacity check, and the planner's allocation
        ExtractAcc acc;
        int kept = 0;
        read_back(stream, {{&acc, dAcc, sizeof(acc)},
                           {&kept, dKept, sizeof(int)},
                           {&out->rootCost, reinterpret_cast<const float*>(tCtrl + root) + 3, sizeof(float)},
                           {deviceOut ? nullptr : newRow, dNewRow, sizeof(int) * (size_t)rows}});
        if ((unsigned)kept != acc.kept)
            throw Error(SBMP_ERR_HIP, "extract: the tile offsets and the summary disagree on the kept rows");
        out->kept = kept;
        out->below = (int)acc.below;
        out->masked = (int)acc.masked;
        out->detached = (int)acc.detached;
        if (!wantMembers) return;
        check_extract_capacity(capacity, kept);
        if (kept == 0) return;
        float* dState = state;
        float* dCtrl = ctrl;
        int* dParent = parent;
        int* dOrigin = origin;
        if (!deviceOut) {
            dState = state ? w.alloc<float>(4 * (size_t)kept) : nullptr;
            dCtrl = ctrl ? w.alloc<float>(4 * (size_t)kept) : nullptr;
            dParent = parent ? w.alloc<int>((size_t)kept) : nullptr;
            dOrigin = origin ? w.alloc<int>((size_t)kept) : nullptr;
        }
        hipLaunchKernelGGL(k_extract_gather, dim3(extract_grid(k_extract_gather, rows, "k_extract_gather")),
                           dim3(kExtractBlock), 0, stream, tState, tCtrl, tParent, (const int*)dNewRow, rows, root,
                           reinterpret_cast<float4*>(dState), reinterpret_cast<float4*>(dCtrl), dParent, dOrigin);
        SBMP_HIP(hipGetLastError());
        if (deviceOut) {
            SBMP_HIP(hipStreamSynchronize(stream));
        } else {
            read_back(stream, {{state, dState, sizeof(float) * 4 * (size_t)kept},
                               {ctrl, dCtrl, sizeof(float) * 4 * (size_t)kept},
                               {parent, dParent, sizeof(int) * (size_t)kept},
                               {origin, dOrigin, sizeof(int) * (size_t)kept}});
        }
    });
}

void tree_extract_batch(const sbmp_tree_extract_args* a, int root, const uint8_t* d_keep, float* d_state, float* d_ctrl,
                        int* d_parent, int* d_origin, int* d_newRow, long long capacity, sbmp_tree_extract* out,
                        hipStream_t stream) {
    check_extract_args(a, root, out);
    KgmtDev d{};
    d.treeState = reinterpret_cast<float4*>(const_cast<float*>(a->state));
    d.treeCtrl = reinterpret_cast<float4*>(const_cast<float*>(a->ctrl));
    d.treeParent = const_cast<int*>(a->parent);
    tree_extract_device(d, a->rows, a->depthBound, root, d_keep, d_state, d_ctrl, d_parent, d_origin, d_newRow, true,
                        capacity, out, stream);
}

void tree_extract_batch_host(const sbmp_tree_extract_args* a, int root, const uint8_t* keep, float* state, float* ctrl,
                             int* parent, int* origin, int* newRow, long long capacity, sbmp_tree_extract* out) {
    check_extract_args(a, root, out);
    std::vector<int> own;
    if (!newRow) {
        own.resize((size_t)a->rows);
        newRow = own.data();
    }
    extract_number_host(a->ctrl, a->parent, a->rows, root, keep, newRow, out);
    if (!state && !ctrl && !parent && !origin) return;
    check_extract_capacity(capacity, out->kept);
    extract_gather_host(a->state, a->ctrl, a->parent, a->rows, root, newRow, state, ctrl, parent, origin);
}

void tree_extract_info(long long rows, sbmp_tree_extract_layout* out) {
    if (!out) throw Error(SBMP_ERR_INVALID_ARGUMENT, "out must be non-NULL");
    if (rows < 0 || rows >= (1ll << 31)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "rows must be in [0, 2^31)");
    out->tileRows = kExtractTileRows;
    out->roundTiles = kExtractRoundTiles;
    out->tiles = extract_tiles(rows);
    out->rounds = (out->tiles + kExtractRoundTiles - 1) / kExtractRoundTiles;
}

}  // namespace sbmp

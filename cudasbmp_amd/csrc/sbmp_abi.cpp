// sbmp_abi.cpp — extern "C" boundary of libsbmp.so (declared in include/sbmp/sbmp.h).
// Every entry point converts exceptions into sbmp_status + a thread-local message.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "kgmt_planner.h"
#include "obstacle_grid.h"
#include "sbmp/sbmp.h"
#include "sbmp/tree_query.h"

using sbmp::Error;
using sbmp::KgmtPlanner;
using sbmp::Planner;

struct sbmp_kgmt {
    Planner* planner = nullptr;
    sbmp::Exchange* comm = nullptr;   // sharded: owned collectives (kgmt_sharded.cpp)
    bool borrowed = false;            // a batch member (sbmp_kgmt_batch_member): the batch plans and owns it
};

struct sbmp_kgmt_batch {
    sbmp::BatchGroup* group = nullptr;
    std::vector<sbmp_kgmt> views;     // one borrowed handle per member
};

namespace sbmp {
Exchange* sharded_create_comm(const uint8_t* id, int nranks, int rank, int device);
Exchange* sharded_create_host_comm(const sbmp_host_collectives& c, int nranks, int rank, int device);
void comm_get_unique_id(uint8_t* id);
void expand_batch(const sbmp_expand_batch_args* args, void* stream);   // batch.hip
void expand_batch_host(const sbmp_expand_batch_args* args);
void insert_batch(const sbmp_insert_batch_args* args, void* stream);
double hbm_copy_bandwidth(size_t bytes, int reps);
void load_system_config(const char* path, sbmp_system_config* out);   // config.cpp
void fold_r2_info(int logSlots, sbmp_fold_info* out);   // fold_batch.cpp
void fold_r2_batch(const uint16_t* d_ring, const int* S, const int* executed, int tFirst, int tLast, int logSlots,
                   int nR2, int rank, int nranks, int* d_valid, int* d_invalid, hipStream_t s);
void fold_r2_batch_host(const uint16_t* ring, const int* S, const int* executed, int tFirst, int tLast, int logSlots,
                        int nR2, int rank, int nranks, int* valid, int* invalid);
}  // namespace sbmp

static thread_local std::string g_last_error;

template <typename F>
static sbmp_status guarded(F&& f) {
    try {
        f();
        return SBMP_OK;
    } catch (const Error& e) {
        g_last_error = e.what();
        return e.status;
    } catch (const std::bad_alloc&) {
        g_last_error = "host out of memory";
        return SBMP_ERR_OUT_OF_MEMORY;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return SBMP_ERR_STATE;
    }
}

#define REQUIRE(cond, msg)                                                   \
    do {                                                                     \
        if (!(cond)) throw Error(SBMP_ERR_INVALID_ARGUMENT, msg);            \
    } while (0)

extern "C" {

int sbmp_abi_version(void) { return SBMP_ABI_VERSION; }

const char* sbmp_status_string(sbmp_status s) {
    switch (s) {
        case SBMP_OK: return "ok";
        case SBMP_ERR_INVALID_ARGUMENT: return "invalid argument";
        case SBMP_ERR_HIP: return "HIP runtime error";
        case SBMP_ERR_IO: return "I/O error";
        case SBMP_ERR_OUT_OF_MEMORY: return "out of memory";
        case SBMP_ERR_STATE: return "invalid state";
        case SBMP_ERR_UNSUPPORTED: return "unsupported";
        case SBMP_ERR_COMM: return "communication error";
        default: return "unknown status";
    }
}

const char* sbmp_last_error(void) { return g_last_error.c_str(); }

sbmp_status sbmp_kgmt_default_params(sbmp_kgmt_params* p) {
    return guarded([&] {
        REQUIRE(p, "params is NULL");
        memset(p, 0, sizeof(*p));
        // reference demos/main.cu:19-28
        p->width = 20.0f;
        p->height = 20.0f;
        p->N = 16;
        p->n = 8;
        p->numIterations = 100;
        p->maxTreeSize = 30000;
        p->numDisc = 10;
        p->agentLength = 1.0f;
        p->goalThreshold = 0.5f;
        p->samplesPerIteration = 0;
        p->agent = SBMP_AGENT_CAR;
        p->fixGNewClear = 0;
        p->device = 0;
        p->profileKernels = 0;
    });
}

sbmp_status sbmp_load_system_config(const char* path, sbmp_system_config* out) {
    return guarded([&] { sbmp::load_system_config(path, out); });
}

sbmp_status sbmp_kgmt_create(const sbmp_kgmt_params* p, sbmp_kgmt** out) {
    return guarded([&] {
        REQUIRE(p && out, "NULL argument");
        *out = nullptr;
        sbmp_kgmt* h = new sbmp_kgmt;
        try {
            h->planner = new KgmtPlanner(*p);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
    });
}

sbmp_status sbmp_kgmt_create_sharded(const sbmp_kgmt_params* p, const uint8_t id[SBMP_COMM_ID_BYTES], int nranks,
                                     int rank, sbmp_kgmt** out) {
    return guarded([&] {
        REQUIRE(p && id && out, "NULL argument");
        REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank/nranks");
        *out = nullptr;
        sbmp_kgmt* h = new sbmp_kgmt;
        try {
            h->comm = sbmp::sharded_create_comm(id, nranks, rank, p->device);
            h->planner = new KgmtPlanner(*p, nranks, rank, h->comm);
        } catch (...) {
            delete h->planner;
            delete h->comm;
            delete h;
            throw;
        }
        *out = h;
    });
}

sbmp_status sbmp_kgmt_create_sharded_host(const sbmp_kgmt_params* p, const sbmp_host_collectives* coll, int nranks,
                                          int rank, sbmp_kgmt** out) {
    return guarded([&] {
        REQUIRE(p && coll && out, "NULL argument");
        REQUIRE(coll->allreduce_u64 && coll->allreduce_i32 && coll->allgather, "NULL collective callback");
        REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank/nranks");
        *out = nullptr;
        sbmp_kgmt* h = new sbmp_kgmt;
        try {
            h->comm = sbmp::sharded_create_host_comm(*coll, nranks, rank, p->device);
            h->planner = new KgmtPlanner(*p, nranks, rank, h->comm);
        } catch (...) {
            delete h->planner;
            delete h->comm;
            delete h;
            throw;
        }
        *out = h;
    });
}

sbmp_status sbmp_kgmt_create_local_group(const sbmp_kgmt_params* p, int nranks, sbmp_kgmt** out) {
    return guarded([&] {
        REQUIRE(p && out, "NULL argument");
        *out = nullptr;
        sbmp_kgmt* h = new sbmp_kgmt;
        try {
            h->planner = (nranks == 1) ? static_cast<Planner*>(new KgmtPlanner(*p))
                                       : static_cast<Planner*>(new sbmp::LocalShardGroup(*p, nranks));
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
    });
}

sbmp_status sbmp_expand_batch(const sbmp_expand_batch_args* args, void* stream) {
    return guarded([&] { sbmp::expand_batch(args, stream); });
}

sbmp_status sbmp_expand_batch_host(const sbmp_expand_batch_args* args) {
    return guarded([&] { sbmp::expand_batch_host(args); });
}

sbmp_status sbmp_insert_batch(const sbmp_insert_batch_args* args, void* stream) {
    return guarded([&] { sbmp::insert_batch(args, stream); });
}

sbmp_status sbmp_tree_query_batch(const float* d_state, const float* d_ctrl, long long rows,
                                  const sbmp_goal_query* goals, int count, sbmp_goal_answer* out, void* stream) {
    return guarded(
        [&] { sbmp::tree_query_device(d_state, d_ctrl, rows, goals, count, out, static_cast<hipStream_t>(stream)); });
}

sbmp_status sbmp_tree_query_batch_host(const float* state, const float* ctrl, long long rows,
                                       const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) {
    return guarded([&] { sbmp::tree_query_host(state, ctrl, rows, goals, count, out); });
}

sbmp_status sbmp_tree_query_alive_batch(const float* d_state, const float* d_ctrl, const uint8_t* d_alive,
                                        long long rows, const sbmp_goal_query* goals, int count,
                                        sbmp_goal_answer* out, void* stream) {
    return guarded([&] {
        sbmp::tree_query_alive_device(d_state, d_ctrl, d_alive, rows, goals, count, out, static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_tree_query_alive_batch_host(const float* state, const float* ctrl, const uint8_t* alive,
                                             long long rows, const sbmp_goal_query* goals, int count,
                                             sbmp_goal_answer* out) {
    return guarded([&] { sbmp::tree_query_alive_host(state, ctrl, alive, rows, goals, count, out); });
}

sbmp_status sbmp_fold_r2_info(int logSlots, sbmp_fold_info* out) {
    return guarded([&] { sbmp::fold_r2_info(logSlots, out); });
}

sbmp_status sbmp_fold_r2_batch(const uint16_t* d_ring, const int* S, const int* executed, int tFirst, int tLast,
                               int logSlots, int nR2, int rank, int nranks, int* d_R2Valid, int* d_R2Invalid,
                               void* stream) {
    return guarded([&] {
        sbmp::fold_r2_batch(d_ring, S, executed, tFirst, tLast, logSlots, nR2, rank, nranks, d_R2Valid, d_R2Invalid,
                            static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_fold_r2_batch_host(const uint16_t* ring, const int* S, const int* executed, int tFirst, int tLast,
                                    int logSlots, int nR2, int rank, int nranks, int* R2Valid, int* R2Invalid) {
    return guarded([&] {
        sbmp::fold_r2_batch_host(ring, S, executed, tFirst, tLast, logSlots, nR2, rank, nranks, R2Valid, R2Invalid);
    });
}

sbmp_status sbmp_tree_recheck_batch(const sbmp_tree_recheck_args* args, uint8_t* status, sbmp_tree_recheck* out,
                                    void* stream) {
    return guarded([&] { sbmp::tree_recheck_batch(args, status, out, static_cast<hipStream_t>(stream)); });
}

sbmp_status sbmp_tree_recheck_batch_host(const sbmp_tree_recheck_args* args, uint8_t* status,
                                         sbmp_tree_recheck* out) {
    return guarded([&] { sbmp::tree_recheck_batch_host(args, status, out); });
}

sbmp_status sbmp_tree_paths_batch(const sbmp_tree_paths_args* args, const int* nodes, int count, int* lengths,
                                  uint8_t* status, int* rows, float* samples, float* costs, long long capacity,
                                  long long* total, void* stream) {
    return guarded([&] {
        sbmp::tree_paths_batch(args, nodes, count, lengths, status, rows, samples, costs, capacity, total,
                               static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_tree_paths_batch_host(const sbmp_tree_paths_args* args, const int* nodes, int count, int* lengths,
                                       uint8_t* status, int* rows, float* samples, float* costs, long long capacity,
                                       long long* total) {
    return guarded(
        [&] { sbmp::tree_paths_batch_host(args, nodes, count, lengths, status, rows, samples, costs, capacity, total); });
}

sbmp_status sbmp_tree_trace_batch(const sbmp_tree_paths_args* args, const int* d_rows, long long count,
                                  float* d_steps, uint8_t* d_status, void* stream) {
    return guarded(
        [&] { sbmp::tree_trace_batch(args, d_rows, count, d_steps, d_status, static_cast<hipStream_t>(stream)); });
}

sbmp_status sbmp_tree_trace_batch_host(const sbmp_tree_paths_args* args, const int* rows, long long count,
                                       float* steps, uint8_t* status) {
    return guarded([&] { sbmp::tree_trace_batch_host(args, rows, count, steps, status); });
}

sbmp_status sbmp_tree_resample_batch(const sbmp_tree_paths_args* args, const int* nodes, int count, double period,
                                     int* counts, uint8_t* status, float* d_states, int* d_edges, double* d_times,
                                     long long capacity, long long* total, void* stream) {
    return guarded([&] {
        sbmp::tree_resample_batch(args, nodes, count, period, counts, status, d_states, d_edges, d_times, capacity, total,
                                  static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_tree_resample_batch_host(const sbmp_tree_paths_args* args, const int* nodes, int count, double period,
                                          int* counts, uint8_t* status, float* states, int* edges, double* times,
                                          long long capacity, long long* total) {
    return guarded([&] {
        sbmp::tree_resample_batch_host(args, nodes, count, period, counts, status, states, edges, times, capacity, total);
    });
}

sbmp_status sbmp_tree_extract_batch(const sbmp_tree_extract_args* args, int root, const uint8_t* d_keep, float* d_state,
                                    float* d_ctrl, int* d_parent, int* d_origin, int* d_newRow, long long capacity,
                                    sbmp_tree_extract* out, void* stream) {
    return guarded([&] {
        sbmp::tree_extract_batch(args, root, d_keep, d_state, d_ctrl, d_parent, d_origin, d_newRow, capacity, out,
                                 static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_tree_extract_batch_host(const sbmp_tree_extract_args* args, int root, const uint8_t* keep, float* state,
                                         float* ctrl, int* parent, int* origin, int* newRow, long long capacity,
                                         sbmp_tree_extract* out) {
    return guarded([&] {
        sbmp::tree_extract_batch_host(args, root, keep, state, ctrl, parent, origin, newRow, capacity, out);
    });
}

sbmp_status sbmp_tree_extract_info(long long rows, sbmp_tree_extract_layout* out) {
    return guarded([&] { sbmp::tree_extract_info(rows, out); });
}

sbmp_status sbmp_goal_radius_threshold(float r, float* t) {
    return guarded([&] {
        REQUIRE(t, "t must be non-NULL");
        *t = sbmp::goal_radius_threshold(r);
    });
}

sbmp_status sbmp_comm_get_unique_id(uint8_t id[SBMP_COMM_ID_BYTES]) {
    return guarded([&] {
        REQUIRE(id, "NULL id");
        sbmp::comm_get_unique_id(id);
    });
}

sbmp_status sbmp_kgmt_destroy(sbmp_kgmt* h) {
    return guarded([&] {
        if (!h) return;
        if (h->borrowed) throw Error(SBMP_ERR_STATE, "a batch member is destroyed with its batch");
        delete h->planner;
        delete h->comm;
        delete h;
    });
}

#define PLANNER(h)                                                     \
    REQUIRE((h) && (h)->planner, "NULL planner handle");               \
    Planner& P = *(h)->planner
// planning calls: a batch member's iterations are driven by its batch
#define OWNED(h)                                                                                        \
    do {                                                                                                \
        if ((h)->borrowed) throw Error(SBMP_ERR_STATE, "a batch member is planned through its batch"); \
    } while (0)

sbmp_status sbmp_kgmt_begin(sbmp_kgmt* h, const float initial[7], const float goal[7], const float* d_obstacles,
                            int obstaclesCount, uint64_t seed) {
    return guarded([&] {
        PLANNER(h);
        OWNED(h);
        P.begin(initial, goal, d_obstacles, obstaclesCount, seed);
    });
}

sbmp_status sbmp_kgmt_plan(sbmp_kgmt* h, const float initial[7], const float goal[7], const float* d_obstacles,
                           int obstaclesCount, uint64_t seed, sbmp_plan_result* result) {
    return guarded([&] {
        PLANNER(h);
        OWNED(h);
        P.begin(initial, goal, d_obstacles, obstaclesCount, seed);
        // The planner's loop control (KgmtPlanner::run_plan): over-enqueued iterations of a
        // finished loop are no-ops, so they cost a few microseconds, not correctness.
        P.run_plan();
        if (result) P.result(result);
    });
}

sbmp_status sbmp_kgmt_step(sbmp_kgmt* h, int iterations, int* active) {
    return guarded([&] {
        PLANNER(h);
        OWNED(h);
        REQUIRE(iterations >= 0, "iterations must be >= 0");
        P.enqueue(iterations);
        const bool a = P.active();
        if (active) *active = a ? 1 : 0;
    });
}

sbmp_status sbmp_kgmt_enqueue(sbmp_kgmt* h, int iterations) {
    return guarded([&] {
        PLANNER(h);
        OWNED(h);
        REQUIRE(iterations >= 0, "iterations must be >= 0");
        P.enqueue(iterations);
    });
}

sbmp_status sbmp_kgmt_sync(sbmp_kgmt* h) {
    return guarded([&] {
        PLANNER(h);
        P.sync();
    });
}

sbmp_status sbmp_kgmt_set_iteration_dump(sbmp_kgmt* h, const char* dir) {
    return guarded([&] {
        PLANNER(h);
        if (h->borrowed) throw Error(SBMP_ERR_UNSUPPORTED, "per-iteration dumps are not supported in a batch");
        P.set_iteration_dump(dir ? std::string(dir) : std::string());
    });
}

sbmp_status sbmp_kgmt_fold(sbmp_kgmt* h) {
    return guarded([&] {
        PLANNER(h);
        P.fold_pending();
    });
}

sbmp_status sbmp_kgmt_result(sbmp_kgmt* h, sbmp_plan_result* result) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(result, "NULL result");
        P.result(result);
    });
}

sbmp_status sbmp_kgmt_stream(sbmp_kgmt* h, void** stream) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(stream, "NULL stream");
        *stream = (void*)P.stream();
    });
}

sbmp_status sbmp_kgmt_copy_tree(sbmp_kgmt* h, float* samples, int* parent, float* costs, int capacity) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(capacity >= P.params().maxTreeSize, "capacity < maxTreeSize");
        P.copy_tree(samples, parent, costs);
    });
}

sbmp_status sbmp_kgmt_copy_unexplored(sbmp_kgmt* h, float* samples, int* uParent, int capacity) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(capacity >= P.params().maxTreeSize, "capacity < maxTreeSize");
        P.copy_unexplored(samples, uParent);
    });
}

sbmp_status sbmp_kgmt_copy_flags(sbmp_kgmt* h, uint8_t* G, uint8_t* GNew, int capacity) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(capacity >= P.params().maxTreeSize, "capacity < maxTreeSize");
        P.copy_flags(G, GNew);
    });
}

sbmp_status sbmp_kgmt_copy_regions(sbmp_kgmt* h, int* R1, int* R1Avail, int* R1Valid, int* R1Invalid, float* R1Score,
                                   int* R2Avail, int* R2Valid, int* R2Invalid) {
    return guarded([&] {
        PLANNER(h);
        P.copy_regions(R1, R1Avail, R1Valid, R1Invalid, R1Score, R2Avail, R2Valid, R2Invalid);
    });
}

sbmp_status sbmp_kgmt_num_slots(sbmp_kgmt* h, int* slots) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(slots, "NULL slots");
        *slots = P.num_slots();
    });
}

sbmp_status sbmp_kgmt_copy_rng(sbmp_kgmt* h, uint32_t* states, int capacity) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(states && capacity >= P.num_slots(), "capacity < num_slots");
        P.copy_rng(states);
    });
}

sbmp_status sbmp_kgmt_iter_log(sbmp_kgmt* h, sbmp_iter_record* out, int capacity, int* count) {
    return guarded([&] {
        PLANNER(h);
        std::vector<sbmp_iter_record> log = P.iter_log();
        const int n = std::min<int>(capacity, (int)log.size());
        if (out && n > 0) memcpy(out, log.data(), sizeof(sbmp_iter_record) * n);
        if (count) *count = (int)log.size();
    });
}

sbmp_status sbmp_kgmt_export_csv(sbmp_kgmt* h, const char* dir) {
    return guarded([&] {
        PLANNER(h);
        P.export_csv(dir ? dir : "");
    });
}

sbmp_status sbmp_kgmt_solution_path(sbmp_kgmt* h, int node, int* rows, float* samples, float* costs, int capacity,
                                    int* length) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(length, "length must be non-NULL");
        const int len = P.solution_path(node, nullptr, nullptr, nullptr, 0);
        *length = len;
        if (!rows && !samples && !costs) return;
        REQUIRE(capacity >= len, "capacity smaller than the path length");
        P.solution_path(node, rows, samples, costs, capacity);
    });
}

sbmp_status sbmp_kgmt_query_goals(sbmp_kgmt* h, const sbmp_goal_query* goals, int count, sbmp_goal_answer* out) {
    return guarded([&] {
        PLANNER(h);
        P.query_goals(goals, count, out);
    });
}

sbmp_status sbmp_kgmt_recheck_tree(sbmp_kgmt* h, const float* d_obstacles, int obstaclesCount, uint8_t* status,
                                   int capacity, sbmp_tree_recheck* out) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(out, "out must be non-NULL");
        REQUIRE(obstaclesCount >= 0, "obstaclesCount must be >= 0");
        REQUIRE(obstaclesCount == 0 || d_obstacles, "NULL obstacle list with obstaclesCount > 0");
        P.recheck_tree(d_obstacles, obstaclesCount, status, capacity, out);
    });
}

sbmp_status sbmp_kgmt_query_goals_alive(sbmp_kgmt* h, const sbmp_goal_query* goals, int count,
                                        sbmp_goal_answer* out) {
    return guarded([&] {
        PLANNER(h);
        P.query_goals_alive(goals, count, out);
    });
}

sbmp_status sbmp_kgmt_solution_paths(sbmp_kgmt* h, const int* nodes, int count, int* lengths, uint8_t* status,
                                     int* rows, float* samples, float* costs, long long capacity, long long* total) {
    return guarded([&] {
        PLANNER(h);
        P.solution_paths(nodes, count, lengths, status, rows, samples, costs, capacity, total);
    });
}

sbmp_status sbmp_kgmt_trace_rows(sbmp_kgmt* h, const int* rows, long long count, float* steps, uint8_t* status) {
    return guarded([&] {
        PLANNER(h);
        P.trace_rows(rows, count, steps, status);
    });
}

sbmp_status sbmp_kgmt_resample_paths(sbmp_kgmt* h, const int* nodes, int count, double period, int* counts,
                                     uint8_t* status, float* states, int* edges, double* times, long long capacity,
                                     long long* total) {
    return guarded([&] {
        PLANNER(h);
        P.resample_paths(nodes, count, period, counts, status, states, edges, times, capacity, total);
    });
}

sbmp_status sbmp_kgmt_extract_tree(sbmp_kgmt* h, int root, int useAlive, float* state, float* ctrl, int* parent,
                                   int* origin, int* newRow, long long capacity, sbmp_tree_extract* out) {
    return guarded([&] {
        PLANNER(h);
        P.extract_tree(root, useAlive != 0, state, ctrl, parent, origin, newRow, capacity, out);
    });
}

sbmp_status sbmp_kgmt_adopt_tree(sbmp_kgmt* h, const sbmp_tree_adopt_args* args, const float goal[7],
                                 const float* d_obstacles, int obstaclesCount, uint64_t seed, sbmp_tree_adopt* out) {
    return guarded([&] {
        PLANNER(h);
        if (h->borrowed) throw Error(SBMP_ERR_STATE, "adopting a tree is not supported on a batch member");
        P.adopt_tree(args, goal, d_obstacles, obstaclesCount, seed, out);
    });
}

sbmp_status sbmp_kgmt_replan(sbmp_kgmt* h, int root, int useAlive, int frontierFrom, const float goal[7],
                             const float* d_obstacles, int obstaclesCount, uint64_t seed, sbmp_tree_adopt* out) {
    return guarded([&] {
        PLANNER(h);
        if (h->borrowed) throw Error(SBMP_ERR_STATE, "replanning by adoption is not supported on a batch member");
        P.replan(root, useAlive != 0, frontierFrom, goal, d_obstacles, obstaclesCount, seed, out);
    });
}

sbmp_status sbmp_kgmt_reanchor_tree(sbmp_kgmt* h, int root, const float newRoot[4], const float* d_obstacles,
                                    int obstaclesCount, float* state, float* ctrl, int* parent, int* origin,
                                    uint8_t* status, long long capacity, sbmp_tree_reanchor* out) {
    return guarded([&] {
        PLANNER(h);
        P.reanchor_tree(root, newRoot, d_obstacles, obstaclesCount, state, ctrl, parent, origin, status, capacity, out);
    });
}

sbmp_status sbmp_kgmt_replan_from(sbmp_kgmt* h, int root, const float newRoot[4], int frontierFrom,
                                  const float goal[7], const float* d_obstacles, int obstaclesCount, uint64_t seed,
                                  sbmp_tree_reanchor* reanchorOut, sbmp_tree_adopt* adoptOut) {
    return guarded([&] {
        PLANNER(h);
        if (h->borrowed) throw Error(SBMP_ERR_STATE, "replanning by adoption is not supported on a batch member");
        P.replan_from(root, newRoot, frontierFrom, goal, d_obstacles, obstaclesCount, seed, reanchorOut, adoptOut);
    });
}

sbmp_status sbmp_tree_reanchor_batch(const sbmp_tree_recheck_args* args, const float newRoot[4], float* d_outState,
                                     uint8_t* d_alive, uint8_t* status, sbmp_tree_reanchor* out, void* stream) {
    return guarded([&] {
        sbmp::tree_reanchor_batch(args, newRoot, d_outState, d_alive, status, out, static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_tree_reanchor_batch_host(const sbmp_tree_recheck_args* args, const float newRoot[4], float* outState,
                                          uint8_t* alive, uint8_t* status, sbmp_tree_reanchor* out) {
    return guarded([&] { sbmp::tree_reanchor_batch_host(args, newRoot, outState, alive, status, out); });
}

sbmp_status sbmp_tree_adopt_tables(const sbmp_tree_adopt_tables_args* args, int* R1, int* R1Avail, int* R1Valid,
                                   int* R1Invalid, int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out, void* stream) {
    return guarded([&] {
        sbmp::tree_adopt_tables_device(args, R1, R1Avail, R1Valid, R1Invalid, R1Cov, R2bits, out,
                                       static_cast<hipStream_t>(stream));
    });
}

sbmp_status sbmp_tree_adopt_tables_host(const sbmp_tree_adopt_tables_args* args, int* R1, int* R1Avail, int* R1Valid,
                                        int* R1Invalid, int* R1Cov, uint32_t* R2bits, sbmp_tree_adopt* out) {
    return guarded([&] { sbmp::tree_adopt_tables_host(args, R1, R1Avail, R1Valid, R1Invalid, R1Cov, R2bits, out); });
}

sbmp_status sbmp_kgmt_kernel_stats(sbmp_kgmt* h, sbmp_kernel_stat* out, int capacity, int* count) {
    return guarded([&] {
        PLANNER(h);
        std::vector<sbmp_kernel_stat> st = P.kernel_stats();
        const int n = std::min<int>(capacity, (int)st.size());
        if (out && n > 0) memcpy(out, st.data(), sizeof(sbmp_kernel_stat) * n);
        if (count) *count = (int)st.size();
    });
}

sbmp_status sbmp_kgmt_path_info(sbmp_kgmt* h, sbmp_path_info* out) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(out, "out must be non-NULL");
        P.path_info(out);
    });
}

sbmp_status sbmp_kgmt_reset_kernel_stats(sbmp_kgmt* h) {
    return guarded([&] {
        PLANNER(h);
        P.reset_kernel_stats();
    });
}

sbmp_status sbmp_kgmt_enqueue_delay(sbmp_kgmt* h, double microseconds) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(microseconds >= 0.0 && microseconds <= 1e6, "delay must be in [0, 1 s]");
        P.enqueue_delay(microseconds);
    });
}

sbmp_status sbmp_kgmt_kernel_samples(sbmp_kgmt* h, const char* name, float* out, int capacity, int* count) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(name, "NULL name");
        std::vector<float> v = P.kernel_samples(name);
        const int n = std::min<int>(capacity, (int)v.size());
        if (out && n > 0) memcpy(out, v.data(), sizeof(float) * n);
        if (count) *count = (int)v.size();
    });
}

sbmp_status sbmp_kgmt_set_profiling(sbmp_kgmt* h, int enabled) {
    return guarded([&] {
        PLANNER(h);
        P.set_profiling(enabled != 0);
    });
}

sbmp_status sbmp_kgmt_state_hash(sbmp_kgmt* h, uint64_t* out) {
    return guarded([&] {
        PLANNER(h);
        REQUIRE(out, "out must be non-NULL");
        *out = (uint64_t)P.state_hash();
    });
}


// readObstaclesFromCSV (reference src/helper/helper.cu:11-34): values separated
// by whitespace or single commas, read line by line with operator>>.
sbmp_status sbmp_read_obstacles_csv(const char* path, int workspaceDim, float* out, int capacity,
                                    int* numObstacles) {
    return guarded([&] {
        REQUIRE(path && numObstacles && workspaceDim > 0, "bad argument");
        std::ifstream file(path);
        if (!file.is_open()) throw Error(SBMP_ERR_IO, std::string("Error opening file: ") + path);
        std::vector<float> v;
        std::string line;
        while (std::getline(file, line)) {
            std::stringstream ss(line);
            float value;
            while (ss >> value) {
                v.push_back(value);
                if (ss.peek() == ',') ss.ignore();
            }
        }
        const int n = (int)(v.size() / (2 * workspaceDim));
        *numObstacles = n;
        if (out) {
            REQUIRE(capacity >= (int)v.size(), "capacity smaller than the file's float count");
            memcpy(out, v.data(), sizeof(float) * v.size());
        }
    });
}

sbmp_status sbmp_random_tree(int device, int kind, const float* root, int rows, int blocks, int threadsPerBlock,
                             float* samples, long long capacity, float* kernelMs) {
    return guarded([&] {
        REQUIRE(root && samples, "root and samples must be non-NULL");
        REQUIRE(kind == SBMP_RANDOM_TREE_NAIVE || kind == SBMP_RANDOM_TREE_COSTPROP, "unknown generator kind");
        const bool naive = kind == SBMP_RANDOM_TREE_NAIVE;
        if (rows <= 0) rows = naive ? 10 : 1;                       // NaivePlanner.cu:80 / CostPropPlanner.cu:87
        if (blocks <= 0) blocks = naive ? 32 : 512;                 // :79 / :86
        if (threadsPerBlock <= 0) threadsPerBlock = naive ? 32 : 1024;   // :78 / :85
        REQUIRE(threadsPerBlock <= 1024, "threadsPerBlock must be <= 1024");
        const long long n = (long long)rows * blocks * threadsPerBlock * 7;
        REQUIRE(n < (1ll << 31), "tree larger than 2^31 floats (the reference indexes it with int)");
        REQUIRE(capacity >= n, "capacity smaller than rows * blocks * threadsPerBlock * 7");
        int ndev = 0;
        SBMP_HIP(hipGetDeviceCount(&ndev));
        REQUIRE(device >= 0 && device < ndev, "no such HIP device");
        sbmp::random_tree(device, kind, root, rows, blocks, threadsPerBlock, samples, kernelMs);
    });
}

sbmp_status sbmp_obstacle_grid_query(const float* obstacles, int nObs, float width, float height, int gridSize,
                                     const float* segments, int nSegments, uint8_t* freeOut, int* gridUsed) {
    return guarded([&] {
        REQUIRE(nObs >= 0 && nSegments >= 0 && (nObs == 0 || obstacles) && (nSegments == 0 || (segments && freeOut)),
                "bad argument");
        REQUIRE(width > 0.0f && height > 0.0f, "width and height must be positive");
        const sbmp::HostObstacleGrid g = sbmp::build_obstacle_grid(obstacles, nObs, width, height, gridSize);
        for (int i = 0; i < nSegments; ++i) {
            const float* q = segments + 4 * i;
            freeOut[i] = sbmp::grid_motion_valid(q[0], q[1], q[2], q[3], g.g, g.invW, g.invH, g.start.data(),
                                                 g.boxes.data())
                             ? 1
                             : 0;
        }
        if (gridUsed) *gridUsed = g.g;
    });
}

sbmp_status sbmp_device_upload_f32(const float* host, size_t count, float** d_out) {
    return guarded([&] {
        REQUIRE(d_out && (host || count == 0), "bad argument");
        void* p = nullptr;
        SBMP_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(float)));
        if (count) {
            hipError_t e = hipMemcpy(p, host, count * sizeof(float), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                hipFree(p);
                SBMP_HIP(e);
            }
        }
        *d_out = static_cast<float*>(p);
    });
}

sbmp_status sbmp_device_free(void* d_ptr) {
    return guarded([&] {
        if (d_ptr) SBMP_HIP(hipFree(d_ptr));
    });
}

sbmp_status sbmp_device_alloc(size_t bytes, void** d_out) {
    return guarded([&] {
        REQUIRE(d_out, "NULL output pointer");
        *d_out = nullptr;
        SBMP_HIP(hipMalloc(d_out, bytes > 0 ? bytes : 1));
    });
}

sbmp_status sbmp_device_copy_to(void* d_dst, const void* host, size_t bytes) {
    return guarded([&] {
        REQUIRE(bytes == 0 || (d_dst && host), "NULL pointer");
        if (bytes) SBMP_HIP(hipMemcpy(d_dst, host, bytes, hipMemcpyHostToDevice));
    });
}

sbmp_status sbmp_device_copy_from(void* host, const void* d_src, size_t bytes) {
    return guarded([&] {
        REQUIRE(bytes == 0 || (d_src && host), "NULL pointer");
        if (bytes) SBMP_HIP(hipMemcpy(host, d_src, bytes, hipMemcpyDeviceToHost));
    });
}

sbmp_status sbmp_device_count(int* count) {
    return guarded([&] {
        REQUIRE(count, "NULL count");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        *count = (e == hipSuccess) ? n : 0;
    });
}

sbmp_status sbmp_hbm_copy_bandwidth(size_t bytes, int reps, double* gbs) {
    return guarded([&] {
        REQUIRE(gbs, "NULL output");
        *gbs = 0.0;
        *gbs = sbmp::hbm_copy_bandwidth(bytes, reps);
    });
}

// ---------------------------------------------------------------- batches
#define BATCH(h)                                                   \
    REQUIRE((h) && (h)->group, "NULL batch handle");               \
    sbmp::BatchGroup& B = *(h)->group

sbmp_status sbmp_kgmt_batch_create(const sbmp_kgmt_params* p, int count, sbmp_kgmt_batch** out) {
    return guarded([&] {
        REQUIRE(p && out, "NULL argument");
        *out = nullptr;
        REQUIRE(count >= 1, "a batch needs at least one member");
        sbmp_kgmt_batch* h = new sbmp_kgmt_batch;
        try {
            h->group = new sbmp::BatchGroup(*p, count);
            h->views.resize(count);
            for (int i = 0; i < count; ++i) {
                h->views[i].planner = &h->group->member(i);
                h->views[i].borrowed = true;
            }
        } catch (...) {
            delete h->group;
            delete h;
            throw;
        }
        *out = h;
    });
}

sbmp_status sbmp_kgmt_batch_destroy(sbmp_kgmt_batch* h) {
    return guarded([&] {
        if (!h) return;
        delete h->group;
        delete h;
    });
}

sbmp_status sbmp_kgmt_batch_begin(sbmp_kgmt_batch* h, const float* initials, const float* goals,
                                  const float* d_obstacles, int obstaclesCount, const uint64_t* seeds) {
    return guarded([&] {
        BATCH(h);
        B.begin(initials, goals, d_obstacles, obstaclesCount, seeds);
    });
}

sbmp_status sbmp_kgmt_batch_plan(sbmp_kgmt_batch* h, const float* initials, const float* goals,
                                 const float* d_obstacles, int obstaclesCount, const uint64_t* seeds,
                                 sbmp_plan_result* results) {
    return guarded([&] {
        BATCH(h);
        B.begin(initials, goals, d_obstacles, obstaclesCount, seeds);
        B.run_plan();
        if (results)
            for (int i = 0; i < B.count(); ++i) B.result(i, results + i);
    });
}

sbmp_status sbmp_kgmt_batch_step(sbmp_kgmt_batch* h, int iterations, int* active) {
    return guarded([&] {
        BATCH(h);
        REQUIRE(iterations >= 0, "iterations must be >= 0");
        B.enqueue(iterations);
        const int a = B.active();
        if (active) *active = a;
    });
}

sbmp_status sbmp_kgmt_batch_enqueue(sbmp_kgmt_batch* h, int iterations) {
    return guarded([&] {
        BATCH(h);
        REQUIRE(iterations >= 0, "iterations must be >= 0");
        B.enqueue(iterations);
    });
}

sbmp_status sbmp_kgmt_batch_sync(sbmp_kgmt_batch* h) {
    return guarded([&] {
        BATCH(h);
        B.sync();
    });
}

sbmp_status sbmp_kgmt_batch_result(sbmp_kgmt_batch* h, int member, sbmp_plan_result* result) {
    return guarded([&] {
        BATCH(h);
        REQUIRE(result, "NULL result");
        B.result(member, result);
    });
}

sbmp_status sbmp_kgmt_batch_member(sbmp_kgmt_batch* h, int i, sbmp_kgmt** borrowed) {
    return guarded([&] {
        BATCH(h);
        REQUIRE(borrowed, "NULL output");
        *borrowed = nullptr;
        REQUIRE(i >= 0 && i < B.count(), "no such batch member");
        *borrowed = &h->views[i];
    });
}

sbmp_status sbmp_kgmt_batch_info(sbmp_kgmt_batch* h, sbmp_batch_info* out) {
    return guarded([&] {
        BATCH(h);
        REQUIRE(out, "out must be non-NULL");
        B.info(out);
    });
}

sbmp_status sbmp_kgmt_batch_kernel_stat(sbmp_kgmt_batch* h, sbmp_kernel_stat* out) {
    return guarded([&] {
        BATCH(h);
        REQUIRE(out, "out must be non-NULL");
        *out = B.kernel_stat();
    });
}

sbmp_status sbmp_batch_pack(const int* groupsPerMember, int count, int residentGroups, int* launchOfMember,
                            int* launches) {
    return guarded([&] {
        REQUIRE(groupsPerMember && launchOfMember && launches, "NULL argument");
        REQUIRE(count >= 1, "count must be >= 1");
        REQUIRE(residentGroups >= 0, "residentGroups must be >= 0");
        for (int i = 0; i < count; ++i) REQUIRE(groupsPerMember[i] >= 1, "a member has at least one workgroup");
        *launches = sbmp::BatchGroup::pack(groupsPerMember, count, residentGroups, launchOfMember);
    });
}

sbmp_status sbmp_division_reciprocal(float b, float* reciprocal) {
    return guarded([&] {
        REQUIRE(reciprocal, "reciprocal must be non-NULL");
        *reciprocal = sbmp::markstein_rcp(b);
    });
}

}  // extern "C"

// kgmt_batch.cpp — BatchGroup: several independent single-rank plans on one device and one
// stream, their k_step launches of an iteration merged into k_step_batch launches
// (kgmt_kernels.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "kgmt_planner.h"

namespace sbmp {

// f() on behalf of member i: an Error it throws names the member.
template <typename F>
static auto for_member(int i, F f) {
    try {
        return f();
    } catch (const Error& e) {
        throw Error(e.status, "member " + std::to_string(i) + ": " + e.what());
    }
}

// Members in index order, each launch filled while the next member still fits: for
// contiguous groups in a fixed order the greedy split has the fewest launches.
int BatchGroup::pack(const int* groupsPerMember, int count, int residentGroups, int* launchOfMember) {
    int launches = 0, used = 0;
    bool open = false;
    for (int i = 0; i < count; ++i) {
        const int g = groupsPerMember[i];
        if (g > residentGroups) {   // does not fit alone: not batchable (and it ends the open launch: index order)
            launchOfMember[i] = -1;
            open = false;
            continue;
        }
        if (!open || used + g > residentGroups) {
            ++launches;
            used = 0;
            open = true;
        }
        used += g;
        launchOfMember[i] = launches - 1;
    }
    return launches;
}

BatchGroup::BatchGroup(const sbmp_kgmt_params& p, int count) : p_(p) {
    if (count < 1) throw Error(SBMP_ERR_INVALID_ARGUMENT, "a batch needs at least one member");
    int ndev = 0;
    SBMP_HIP(hipGetDeviceCount(&ndev));
    if (p.device < 0 || p.device >= ndev) throw Error(SBMP_ERR_INVALID_ARGUMENT, "no such HIP device");
    SBMP_HIP(hipSetDevice(p.device));
    SBMP_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    try {
        for (int i = 0; i < count; ++i) members_.push_back(new KgmtPlanner(p, 1, 0, nullptr, stream_));
    } catch (...) {
        for (KgmtPlanner* k : members_) delete k;
        (void)hipStreamDestroy(stream_);
        throw;
    }
    launchOf_.assign(count, -1);
    groupsPerMember_ = 1 + members_[0]->d_.nBlocks;
}

void BatchGroup::free_launches() {
    for (Launch& l : launches_) {
        if (l.dTable) (void)hipFree(l.dTable);
        if (l.stage) (void)hipHostFree(l.stage);
    }
    launches_.clear();
}

BatchGroup::~BatchGroup() {
    (void)hipSetDevice(p_.device);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (KgmtPlanner* k : members_) delete k;
    free_launches();
    if (stream_) (void)hipStreamDestroy(stream_);
}

KgmtPlanner& BatchGroup::member(int i) {
    if (i < 0 || i >= count()) throw Error(SBMP_ERR_INVALID_ARGUMENT, "no such batch member");
    return *members_[i];
}

void BatchGroup::begin(const float* initials, const float* goals, const float* d_obstacles, int nObs,
                       const uint64_t* seeds) {
    if (!initials || !goals || !seeds) throw Error(SBMP_ERR_INVALID_ARGUMENT, "initials/goals/seeds must be non-NULL");
    const int B = count();
    for (int m = 0; m < B; ++m)   // every member's arguments before anything is launched
        for_member(m, [&] { KgmtPlanner::check_begin_args(initials + 7 * m, goals + 7 * m, d_obstacles, nObs); });
    SBMP_HIP(hipSetDevice(p_.device));
    begun_ = false;
    for (int m = 0; m < B; ++m) members_[m]->begin(initials + 7 * m, goals + 7 * m, d_obstacles, nObs, seeds[m]);
    // One parameter set and one list: every member chose the same form.
    bool step = true;
    for (KgmtPlanner* k : members_) step = step && k->d_.stepMode && k->d_.hostPoll;
    for (KgmtPlanner* k : members_)
        if ((k->d_.stepMode != 0) != (members_[0]->d_.stepMode != 0))
            throw Error(SBMP_ERR_STATE, "batch members chose different forms");
    residentGroups_ = 0;
    membersPerLaunch_ = 1;
    std::fill(launchOf_.begin(), launchOf_.end(), -1);
    int nLaunches = 0;
    if (step) {
        // the occupancy of k_step_batch itself (its registers need not equal k_step's), at
        // this plan's dynamic LDS; SBMP_BATCH_MAX_GROUPS lowers it (tests: the split path)
        KgmtPlanner& k0 = *members_[0];
        residentGroups_ = step_batch_resident_groups(k0.d_, k0.p_.agent, k0.expandVariant_);
        if (const char* v = getenv("SBMP_BATCH_MAX_GROUPS")) {
            const int cap = atoi(v);
            if (cap >= 0 && cap < residentGroups_) residentGroups_ = cap;
        }
        std::vector<int> groups(B);
        for (int m = 0; m < B; ++m) groups[m] = 1 + members_[m]->d_.nBlocks;
        nLaunches = pack(groups.data(), B, residentGroups_, launchOf_.data());
        if (nLaunches == 0 || std::count(launchOf_.begin(), launchOf_.end(), -1) > 0) {
            // a member does not fit alone (the members are equal, so none does): the
            // two-launch form, which needs no residency; k_finish(0) prepares iteration 1
            for (KgmtPlanner* k : members_) {
                k->d_.stepMode = 0;
                k->flushed_ = true;
                launch_finish(k->d_, 0, 0, stream_, k->timing(KgmtPlanner::K_FINISH));
            }
            SBMP_HIP(hipGetLastError());
            step = false;
            nLaunches = 0;
        }
    }
    batched_ = step;
    // the launches' tables: member ranges are contiguous (index order)
    bool same = (int)launches_.size() == nLaunches;
    if (same) {
        std::vector<int> cnt(nLaunches, 0);
        for (int m = 0; m < B && batched_; ++m) cnt[launchOf_[m]]++;
        for (int l = 0; l < nLaunches; ++l) same = same && launches_[l].members == cnt[l];
    }
    if (!same) {
        SBMP_HIP(hipStreamSynchronize(stream_));
        free_launches();
        launches_.resize(nLaunches);
        for (int m = 0; m < B && batched_; ++m) {
            Launch& l = launches_[launchOf_[m]];
            if (l.members == 0) l.first = m;
            l.members++;
        }
        for (Launch& l : launches_) {
            SBMP_HIP(hipMalloc(reinterpret_cast<void**>(&l.dTable), sizeof(StepBatchRec) * l.members));
            SBMP_HIP(hipHostMalloc(reinterpret_cast<void**>(&l.stage), sizeof(StepBatchRec) * l.members,
                                   hipHostMallocDefault));
        }
    }
    for (Launch& l : launches_) {
        l.maxGroups = 0;
        for (int m = l.first; m < l.first + l.members; ++m)
            l.maxGroups = std::max(l.maxGroups, 1 + members_[m]->d_.nBlocks);
        membersPerLaunch_ = std::max(membersPerLaunch_, l.members);
    }
    // The launches' tables, written once per plan: nothing in a record changes with the
    // iteration (t and the expand flag are a kernel argument).  Every member's begin()
    // drained the stream, so no earlier copy from the staging tables is queued.
    if (batched_) {
        for (KgmtPlanner* k : members_) k->upload_dev();
        for (Launch& l : launches_) {
            for (int i = 0; i < l.members; ++i) step_batch_record(members_[l.first + i]->d_, l.stage + i);
            SBMP_HIP(hipMemcpyAsync(l.dTable, l.stage, sizeof(StepBatchRec) * l.members, hipMemcpyHostToDevice, stream_));
        }
        SBMP_HIP(hipStreamSynchronize(stream_));   // outside the plan's wall time, like the rest of begin()
    }
    const double t0 = now_ms();   // one start for the batch: a member's wallMs runs to its own end
    for (KgmtPlanner* k : members_) k->t0_ = t0;
    begun_ = true;
}

// The batch launches of iteration t (expand == 0: its flush pass), back to back.
void BatchGroup::issue(int t, int expand) {
    for (Launch& l : launches_) {
        KgmtPlanner& k0 = *members_[l.first];
        launch_step_batch(k0.d_, t, expand, k0.p_.agent, k0.expandVariant_, l.dTable, l.members, l.maxGroups, stream_,
                          expand ? timer_.take(0, members_[0]->p_.profileKernels != 0) : KernelTiming());
    }
}

void BatchGroup::stage_member(KgmtPlanner* k, int t) {
    if (k->d_.stepMode) {
        k->stage_step(t);
    } else {
        k->stage_expand(t);
        k->stage_finish(t);
    }
}

void BatchGroup::enqueue(int iterations) {
    if (!begun_) throw Error(SBMP_ERR_STATE, "begin() has not been called");
    for (int i = 0; i < iterations; ++i) {
        int t = 0;
        for (KgmtPlanner* k : members_) t = k->take_iteration();   // all members advance together
        if (t == 0) break;
        if (batched_) {
            for (KgmtPlanner* k : members_) k->upload_dev();
            issue(t, 1);
            for (KgmtPlanner* k : members_) k->flushed_ = false;
        } else {
            for (KgmtPlanner* k : members_) stage_member(k, t);
        }
        for (KgmtPlanner* k : members_) k->stage_fold(t);
    }
    SBMP_HIP(hipGetLastError());
}

// The members' flush passes (insert the last iteration, plan the next) as batch launches.
void BatchGroup::flush() {
    if (!begun_) return;
    if (batched_) {
        bool any = false;
        for (KgmtPlanner* k : members_) any = any || !k->flushed_;
        if (!any) return;
        for (KgmtPlanner* k : members_) k->upload_dev();
        issue(members_[0]->t_next_, 0);   // idempotent for a member already flushed
        for (KgmtPlanner* k : members_) k->flushed_ = true;
    } else {
        for (KgmtPlanner* k : members_) k->flush();
    }
}

void BatchGroup::sync() {
    flush();
    for (KgmtPlanner* k : members_) k->sync();   // the first waits for the stream; each takes its wallMs
}

void BatchGroup::fold_pending() {
    for (KgmtPlanner* k : members_) k->fold_pending();
}

int BatchGroup::active() {
    if (!begun_) return 0;
    flush();
    int n = 0;
    for (int m = 0; m < count(); ++m)
        if (for_member(m, [&] { return members_[m]->active(); })) ++n;
    return n;
}

// plan(): KgmtPlanner::run_to_goal over the members, an iteration of all of them per step.
void BatchGroup::run_plan() {
    if (!begun_) throw Error(SBMP_ERR_STATE, "begin() has not been called");
    if (!batched_) {   // the members' own launches in turn, polled as Planner::run does
        while (true) {
            enqueue(8);
            if (active() == 0) break;
        }
        sync();
        return;
    }
    KgmtPlanner::run_to_goal(members_.data(), count(), [this] { enqueue(1); }, [this] { sync(); },
                             [](int m, int e) { for_member(m, [e] { throw_wait_error(e); }); });
}

void BatchGroup::result(int i, sbmp_plan_result* r) {
    KgmtPlanner& k = member(i);
    flush();
    for_member(i, [&] { k.result(r); });
}

void BatchGroup::info(sbmp_batch_info* out) const {
    out->count = count();
    out->groupsPerMember = groupsPerMember_;
    out->residentGroups = residentGroups_;
    out->membersPerLaunch = batched_ ? membersPerLaunch_ : 1;
    out->launchesPerIteration = batched_ ? (int)launches_.size() : count();
    out->batched = batched_ ? 1 : 0;
}

sbmp_kernel_stat BatchGroup::kernel_stat() {
    timer_.collect();
    sbmp_kernel_stat s;
    memset(&s, 0, sizeof(s));
    strncpy(s.name, "k_step_batch", sizeof(s.name) - 1);
    s.launches = timer_.launches(0);
    s.totalMs = timer_.total_ms(0);
    return s;
}

}  // namespace sbmp

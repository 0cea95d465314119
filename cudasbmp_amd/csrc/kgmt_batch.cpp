// kgmt_batch.cpp — BatchGroup: several independent single-rank plans on one device and one
// stream, their k_step launches of an iteration merged into k_step_batch launches
// (kgmt_kernels.hip).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "kgmt_planner.h"

namespace sbmp {

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
    for (auto& q : pending_) {
        (void)hipEventDestroy(q.a);
        (void)hipEventDestroy(q.b);
    }
    for (hipEvent_t e : eventPool_) (void)hipEventDestroy(e);
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
    if (nObs < 0 || (nObs > 0 && !d_obstacles)) throw Error(SBMP_ERR_INVALID_ARGUMENT, "bad obstacles");
    const int B = count();
    for (int m = 0; m < B; ++m)   // D15, for every member before anything is launched
        for (int i = 0; i < 4; ++i)
            if (!std::isfinite(initials[7 * m + i]))
                throw Error(SBMP_ERR_INVALID_ARGUMENT,
                            "member " + std::to_string(m) + ": initial state (x, y, theta, v) must be finite");
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

// The lowest iteration whose planner workgroup has run, over the members (their pinned
// poll words): every launch (and table copy) of an earlier iteration has completed.
int BatchGroup::min_seen() const {
    int lo = INT_MAX;
    for (const KgmtPlanner* k : members_) {
        const unsigned long long v = *const_cast<const volatile unsigned long long*>(&k->poll_->word);
        lo = std::min(lo, (int)(v >> 2));
    }
    return lo;
}

// The batch launches of iteration t (expand == 0: its flush pass), back to back.
void BatchGroup::issue(int t, int expand) {
    for (Launch& l : launches_) {
        KgmtPlanner& k0 = *members_[l.first];
        launch_step_batch(k0.d_, t, expand, k0.p_.agent, k0.expandVariant_, l.dTable, l.members, l.maxGroups, stream_,
                          expand ? timing() : KernelTiming());
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
    for (int m = 0; m < count(); ++m) {
        try {
            if (members_[m]->active()) ++n;
        } catch (const Error& e) {
            throw Error(e.status, "member " + std::to_string(m) + ": " + e.what());
        }
    }
    return n;
}

// plan(): KgmtPlanner::run_to_goal for every member at once.  kAhead iterations stay in
// flight behind the slowest member's planner; a member has ended when its planner's word
// says so (goal, or loop end), and its wallMs is taken once that launch has ended (a later
// launch's planner has stored its word, or the stream is idle).  A finished member stays in
// the later tables: its workgroups are no-ops.
void BatchGroup::run_plan() {
    if (!begun_) throw Error(SBMP_ERR_STATE, "begin() has not been called");
    const int B = count();
    if (!batched_) {   // the members' own launches in turn, polled as Planner::run does
        while (true) {
            enqueue(8);
            if (active() == 0) break;
        }
        sync();
        return;
    }
#ifndef SBMP_PLAN_AHEAD
#define SBMP_PLAN_AHEAD 3
#endif
    constexpr int kAhead = SBMP_PLAN_AHEAD;
    const int numIterations = p_.numIterations;
    std::vector<int> endSeen(B, -1);   // the launch whose planner first reported member m's end
    std::vector<char> fixed(B, 0);
    int issued = members_[0]->t_next_ - 1;
    while (true) {
        int minSeen = INT_MAX, waiting = 0, reported = 0;
        for (int m = 0; m < B; ++m) {
            KgmtPlanner* k = members_[m];
            const unsigned long long v = *const_cast<const volatile unsigned long long*>(&k->poll_->word);
            const int seen = (int)(v >> 2);
            minSeen = std::min(minSeen, seen);
            if (endSeen[m] < 0 && (v & 3ull)) endSeen[m] = seen;
            if (endSeen[m] >= 0) ++reported;
            if (endSeen[m] >= 0 && !fixed[m]) {
                if (seen > endSeen[m]) {
                    k->wallMs_ = now_ms() - k->t0_;
                    k->wallFixed_ = true;
                    fixed[m] = 1;
                } else {
                    ++waiting;
                }
            }
        }
        if (waiting && hipStreamQuery(stream_) != hipErrorNotReady) {   // idle (or failed: sync() raises it)
            for (int m = 0; m < B; ++m)
                if (endSeen[m] >= 0 && !fixed[m]) {
                    members_[m]->wallMs_ = now_ms() - members_[m]->t0_;
                    members_[m]->wallFixed_ = true;
                    fixed[m] = 1;
                }
            waiting = 0;
        }
        if (reported == B) {
            if (!waiting) break;
        } else if (members_[0]->t_next_ <= numIterations && issued - minSeen < kAhead) {
            enqueue(1);
            ++issued;
            continue;
        } else if (members_[0]->t_next_ > numIterations) {
            break;   // every iteration launched: sync() ends it
        } else {   // the stream drained (or failed) without the words this loop waits for: sync() decides
            const hipError_t q = hipStreamQuery(stream_);
            if (q != hipErrorNotReady && (q != hipSuccess || min_seen() < issued)) break;
        }
        __builtin_ia32_pause();
    }
    sync();
    // a bounded in-kernel wait that gave up: raised here, whether or not a result is read
    for (KgmtPlanner* k : members_)
        SBMP_HIP(hipMemcpyAsync(&k->poll_->status, k->d_.status, sizeof(PlannerStatus), hipMemcpyDeviceToHost, stream_));
    SBMP_HIP(hipStreamSynchronize(stream_));
    for (int m = 0; m < B; ++m) {
        if (!members_[m]->poll_->status.error) continue;
        try {
            throw_wait_error(members_[m]->poll_->status.error);
        } catch (const Error& e) {
            throw Error(e.status, "member " + std::to_string(m) + ": " + e.what());
        }
    }
}

void BatchGroup::result(int i, sbmp_plan_result* r) {
    KgmtPlanner& k = member(i);
    flush();
    try {
        k.result(r);
    } catch (const Error& e) {
        throw Error(e.status, "member " + std::to_string(i) + ": " + e.what());
    }
}

void BatchGroup::info(sbmp_batch_info* out) const {
    out->count = count();
    out->groupsPerMember = groupsPerMember_;
    out->residentGroups = residentGroups_;
    out->membersPerLaunch = batched_ ? membersPerLaunch_ : 1;
    out->launchesPerIteration = batched_ ? (int)launches_.size() : count();
    out->batched = batched_ ? 1 : 0;
}

// ---------------------------------------------------------------- profiling
KernelTiming BatchGroup::timing() {
    KernelTiming tm;
    if (!members_[0]->p_.profileKernels) return tm;
    for (hipEvent_t* e : {&tm.start, &tm.stop}) {
        if (!eventPool_.empty()) {
            *e = eventPool_.back();
            eventPool_.pop_back();
        } else {
            SBMP_HIP(hipEventCreate(e));
        }
    }
    pending_.push_back({tm.start, tm.stop});
    return tm;
}

void BatchGroup::collect_events() {
    for (auto& q : pending_) {
        SBMP_HIP(hipEventSynchronize(q.b));
        float ms = 0.0f;
        SBMP_HIP(hipEventElapsedTime(&ms, q.a, q.b));
        statLaunches_ += 1;
        statMs_ += ms;
        eventPool_.push_back(q.a);
        eventPool_.push_back(q.b);
    }
    pending_.clear();
}

sbmp_kernel_stat BatchGroup::kernel_stat() {
    collect_events();
    sbmp_kernel_stat s;
    memset(&s, 0, sizeof(s));
    strncpy(s.name, "k_step_batch", sizeof(s.name) - 1);
    s.launches = statLaunches_;
    s.totalMs = statMs_;
    return s;
}

}  // namespace sbmp

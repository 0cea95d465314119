// kgmt_step_body.h — the body of k_step(t), included (not called) where it runs:
// in k_step itself, whose twelve arguments are the names used here, and in step_body,
// the function form k_step_batch calls with a member's arguments (kgmt_kernels.hip).
// Textual inclusion keeps k_step the very kernel it was before k_step_batch existed: with
// k_step calling the function form too, the same statements compiled to another schedule
// and measured 1-2% slower.  The workgroup's index within its problem is
// blockIdx.x in both kernels (0 plans, 1.. expand).
// Expects: template parameters AGENT, OBS, SH; dp, tx, shRR, cnt4, ctrlPrev, rngAArg,
// rngBArg, gnewArg, statusArg, tlBase, shRows, shBw.  No include guard: included twice.
    const int t = tx & 0x7fffffff, expand = (int)((unsigned)tx >> 31);
    const KgmtDev& d = *dp;
    const ShardView sv{SH ? (shRR >> 8) : 1, SH ? (shRR & 0xff) : 0, SH ? shRows : 0, G(shBw)};
    extern __shared__ float4 sDyn[];   // [LDS obstacles][prefix: nBlocks + 1 ints][R2New bits: nR2 / 32]
    __shared__ int sR1P[kMaxR1];
    __shared__ StepPlan sPlan;
    __shared__ int sWaveCnt[kBlock / kWave];
    __shared__ int sWaveGoal[kBlock / kWave];
    __shared__ int sRed[2][kBlock / kWave];
    __shared__ float sPart[8];
    __shared__ int sCovInc[kMaxR1];

    constexpr bool kLdsObs = (OBS == kObsLds || OBS == kObsLds4);
    constexpr int kRegObs = obs_in_registers(OBS);
    int* const sPfx = reinterpret_cast<int*>(sDyn + (kLdsObs ? d.nObs : 0));
    uint32_t* const sNew = reinterpret_cast<uint32_t*>(sPfx + (SH ? sv.nRows : d.nBlocks) + 1);
    // sharded: the u16 block counts of every row, 16-B aligned after the R2New bits (step_lds_bytes)
    uint16_t* const sC16 = reinterpret_cast<uint16_t*>(sPfx + ((((SH ? sv.nRows : d.nBlocks) + 1 + (d.nR2 >> 5)) + 3) & ~3));
    if (blockIdx.x == 0) {
        step_planner<SH>(d, sv, t, expand, sPfx, sRed, sCovInc, sPart, sC16);
        if constexpr (SH) {
            if (expand && d.fusedX) step_planner_arrive(d, t);
        }
        return;
    }
    float4* const sObs = sDyn;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform
    __shared__ int2 sWaveDiv[kBlock / kWave];   // (frontier position, remainder) of each wave's first slot
    const int b = (int)blockIdx.x - 1;                // this workgroup's 256-slot block (owned index)
    const int gb = SH ? sv.rank + sv.nranks * b : b;   // global block
    const int slot = gb * kBlock + tid;
    const int nW = d.nR2 >> 5;
    const int pp = (t - 1) & 1, cp = t & 1;
    const SBMP_GAS unsigned long long* const pubCur = G(d.stepPub) + (size_t)cp * (d.nR1 + nW);
    // d.timeline if this launch is the traced one (decided on the host: no dependent
    // loads of the plan struct before the prologue's own).  Only a diagnostic build
    // (SBMP_HIPCC_FLAGS=-DSBMP_TIMELINE, tools/mk_variant.sh tl) stamps: held in registers, the
    // eight 64-bit stamps cost every wave ~30 VALU of zeroing and moves.
#ifdef SBMP_TIMELINE
    long long* const tl = tlBase ? tlBase + ((size_t)b * (kBlock / kWave) + wave) * kTimelineStamps : nullptr;
#else
    long long* const tl = nullptr;
    (void)tlBase;
#endif
    long long stamp[kTimelineStamps] = {0, 0, 0, 0, 0, 0, 0, 0};
#define SBMP_STAMP(i)                                                                  \
    do {                                                                               \
        if (tl) stamp[i] = (long long)__builtin_amdgcn_s_memrealtime();                \
    } while (0)
    // The first loads' pointers are preloaded arguments; the plan's scalars and the
    // next pointers in one batch of scalar loads from the struct (one round trip, in
    // flight with the vector loads below)
    const SBMP_GAS IterCtrl* const ctrlP = G(ctrlPrev);
    const SBMP_GAS PlannerStatus* const statusP = G(statusArg);
    const SBMP_GAS uint4* const rngAP = G(rngAArg);
    const SBMP_GAS uint2* const rngBP = G(rngBArg);
    const SBMP_GAS unsigned long long* const gnewP = G(gnewArg);
    SBMP_STAMP(0);

    // ---- loads that depend on nothing else (the control block as a plain load: a
    // waiting scalar load would serialise behind the scan)
    const int4 pk = G(cnt4)[tid];
    const IterCtrl pc = *ctrlP;
    C16Load c16;   // sharded: the u16 block counts of every row (row positions, inserts)
    if constexpr (SH) c16 = c16_issue(d);
    const int goalIdx = statusP->goalIdx;
    const uint4 ra = rngAP[slot];
    const uint2 rb = rngBP[slot];
    const unsigned long long oldWord = (lane == 0) ? gnewP[slot >> 6] : 0ull;
    asm volatile("" ::"s"(d.M), "s"(d.nBlocks), "s"(d.numIterations), "s"(d.numDisc), "s"(d.nR1), "s"(d.nR2),
                 "s"(d.cap), "s"(d.fixGNewClear), "s"(d.batchRule), "s"(d.rcpNumDisc), "s"(d.treeState),
                 "s"(d.treeCtrl), "s"(d.stepList));
    float4 obsReg = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kLdsObs && tid < d.nObs) obsReg = G(d.obstacles)[tid];
    // register lists: box (lane % n) for the per-step schedule (car_schedule)
    float4 oLane = make_float4(0.f, 0.f, 0.f, 0.f);
    if (AGENT == 0 && kRegObs > 0) oLane = G(d.obstacles)[lane % (kRegObs > 0 ? kRegObs : 1)];
    sR1P[tid] = 0;   // nR1 == kBlock
    if (nW <= 2 * kBlock) {   // n <= 8 (uniform): two fixed stores, no loop
        if (tid < nW) sNew[tid] = 0u;
        if (tid + kBlock < nW) sNew[tid + kBlock] = 0u;
    } else {
        for (int i = tid; i < nW; i += kBlock) sNew[i] = 0u;
    }
    // ---- the child's controls (statePropagator.cu:17-21) depend on the slot's stream
    // alone.  Drawn after the count scan (round 6): waves 1-3 while wave 0 plans, wave 0
    // right after the plan's barrier.  Drawn before the scan (rounds 3-5) they held the
    // scan behind the XORWOW states' arrival, the launch's 6.3 MB burst, although the
    // 4-KB counts arrive first: count scan done 2.02 -> 1.32 us p50, every later phase
    // ~0.55 us earlier (profiles/r06/prologue/).
    Xorwow rs{ra.x, ra.y, ra.z, ra.w, rb.x, rb.y};
    ChildCtl ctl;
    auto draw = [&]() __attribute__((always_inline)) {
        ctl = draw_controls<AGENT>(rs, d);
        asm volatile("" : "+v"(ctl.a), "+v"(ctl.steer), "+v"(ctl.dur), "+v"(ctl.dt), "+v"(ctl.tanS));
    };
#if SBMP_VALU_DUP == 1   // diagnostics (VALU by part): the draw once more, on an opaque copy
    {
        Xorwow r2{ra.x, ra.y, ra.z, ra.w, rb.x, rb.y};
        asm volatile("" : "+v"(r2.v0), "+v"(r2.v1), "+v"(r2.v2), "+v"(r2.v3), "+v"(r2.v4), "+v"(r2.d));
        const ChildCtl c2 = draw_controls<AGENT>(r2, d);
        asm volatile("" ::"v"(c2.a), "v"(c2.steer), "v"(c2.dur), "v"(c2.dt), "v"(c2.tanS), "v"(r2.v4), "v"(r2.d));
    }
#endif
    int A, jGoal;
    // the control block and the goal index were loaded per lane (vector loads do not
    // wait behind the scan's scalar work); the plan is wave-uniform, so scalar code
    auto plan = [&]() {
        IterCtrl pcu = pc;
        pcu.executed = __builtin_amdgcn_readfirstlane(pc.executed);
        pcu.treeSize = __builtin_amdgcn_readfirstlane(pc.treeSize);
        pcu.gLo = __builtin_amdgcn_readfirstlane(pc.gLo);
        pcu.nExp = __builtin_amdgcn_readfirstlane(pc.nExp);
        pcu.H = __builtin_amdgcn_readfirstlane(pc.H);
        return step_plan(d, t, expand, pcu, __builtin_amdgcn_readfirstlane(goalIdx), A, jGoal);
    };
    StepPlan q;
    {
        if constexpr (SH) {
            int gRow;
            step_scan_rows(sv, pk, sPfx, sRed, &A, &gRow);
            c16_store(d, c16, sC16);   // published by the plan's barrier below
            if (gRow != kNoGoalIdx) __syncthreads();   // uniform (rare): row_goal reads sPfx[gRow]
            jGoal = row_goal(sv, sPfx, gRow);
        } else {
            step_scan(d, pk, sPfx, sRed, &A, &jGoal);
        }
        SBMP_STAMP(1);
        // One wave per workgroup computes the plan while the others write their prefix
        // entries; the barrier that publishes sPfx publishes the plan.  (Every wave
        // computing it kept the CU's one scalar unit busy for 16 waves at once.)
        if (wave == 0) {
            const StepPlan q0 = plan();
            if (lane == 0) sPlan = q0;
            // slot = g k + i for the first slot of each wave, one division for all four
            // (k >= 64: a wave's slots then span at most two frontier positions)
            if (lane < kBlock / kWave && q0.k >= kWave) {
                const int s0 = gb * kBlock + lane * kWave;
                const int g0 = slot_div(d, s0, q0.k);
                sWaveDiv[lane] = make_int2(g0, s0 - g0 * q0.k);
            }
        }
        else {   // waves 1-3 draw their controls while wave 0 plans
            draw();
        }
        __syncthreads();
        if (wave == 0) draw();
        q = uniform_plan(sPlan);
#ifdef SBMP_TL_PROLOGUE   // diagnostics: stamp 4 = after the plan's barrier (instead of the hand-off)
        SBMP_STAMP(4);
#endif
    }
    // the fused exchange's arrival (every exit of an expanding workgroup)
    auto fx_exit = [&]() {
        if constexpr (SH) {
            if (expand && d.fusedX) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores have completed
                __syncthreads();
                k_step_exchange(d, sv.nranks, sv.rank, sv.nRows, t);
            }
        }
    };
    // the workgroup's work; every exit of it then passes the fused exchange's arrival once
    auto body = [&]() __attribute__((always_inline)) {
    if (!q.ranPrev) return;

    // ---- D6 clear of this block's words of t-1
    const long long cleared = d6_cleared(d.fixGNewClear, q.grid);
    unsigned long long word = oldWord;
    if (d.fixGNewClear) {   // the complete clear: every word (uniform branch)
        word = 0ull;
    } else if (lane == 0) {
        word = d6_clear_word(oldWord, slot >> 6, cleared);
    }
    const bool doExpand = q.executes && gb * kBlock < q.H;
    // ---- insert t-1: this block's flagged children (rows treeSize(t-1) + prefix +
    // index).  Each entry carries its cost, so this is one load and three stores; an
    // expanding block issues it right behind its parent loads (one round trip).
    const bool selfInsert = A > kPlannerInsertMax;   // else the planner workgroup inserts
    auto insert_block = [&](int lo, int j0, int cnt) {   // t-1's flagged children of global block lo: rows j0 ..
        if (tid < cnt) {
            const int j = j0 + tid;
            const int dst = q.tsPrev + j;
            if (j < q.nIns && dst < d.M) {   // D13: the reference writes past M here
                const SBMP_GAS float4* e = list_entry<SH>(d, pp, lo, tid);
                const float4 s4 = list_load<SH>(d, e);
                const float4 u4 = list_load<SH>(d, e + 1);
                const float4 m4 = list_load<SH>(d, e + 2);
                put_row(d, q.tsPrev, j, s4, u4, m4.x);
            }
        }
    };
    auto insert_prev = [&]() {
        if (t > 1 && selfInsert) {
            if constexpr (SH) {   // every rank holds the whole tree: row b = blocks b P .. b P + P - 1
                // the row's entries over the workgroup's lanes (one round of loads for up to
                // 256 entries, whichever of the P blocks holds them)
                const int j0 = sPfx[b], tot = sPfx[b + 1] - j0;
                for (int o = tid; o < tot; o += kBlock) {
                    const int j = j0 + o, dst = q.tsPrev + j;
                    if (j < q.nIns && dst < d.M) {   // D13: the reference writes past M here
                        int blk, idx;
                        row_locate_any(d, sv, sC16, b, o, &blk, &idx);
                        const SBMP_GAS float4* e = list_entry<SH>(d, pp, blk, idx);
                        const float4 s4 = list_load<SH>(d, e);
                        const float4 u4 = list_load<SH>(d, e + 1);
                        const float4 m4 = list_load<SH>(d, e + 2);
                        put_row(d, q.tsPrev, j, s4, u4, m4.x);
                    }
                }
            } else {
                insert_block(b, sPfx[b], sPfx[b + 1] - sPfx[b]);
            }
        }
    };
    if (!doExpand) {
        insert_prev();
        if (lane == 0 && word != oldWord) store_wt(d.gnewOut, slot >> 6, word);
        return;
    }

    // ---- expand t
    const bool act = slot < q.S;
    int g;   // slot = g*k + i
    if (q.k >= kWave) {
        const int2 gr = sWaveDiv[wave];
        g = gr.x + ((gr.y + lane >= q.k) ? 1 : 0);
    } else {
        g = slot_div(d, slot, q.k);
    }
    g = act ? g : 0;
    const int parent = act ? q.gLo + g : 0;
    const SBMP_GAS float4* src = G(d.treeState) + parent;   // the parent's state, and its cost
    const SBMP_GAS float* srcCost = &G(d.treeCtrl)[parent].w;
    // A parent inserted by t-1 is read from its block's compacted list: block lo with
    // sPfx[lo] <= j < sPfx[lo + 1].  j grows with the lane; when a wave's parents are
    // at most two consecutive list positions jA, jB (k >= 32 children per parent) both
    // are found by a two-level 32-ary ballot search (lanes 0-31 for jA, 32-63 for jB):
    // two dependent LDS reads instead of log2(nBlocks).
    const bool fromList = parent >= q.tsPrev;
    const int j = parent - q.tsPrev;
    const unsigned long long need = __ballot(fromList);
    const int nS = SH ? sv.nRows : d.nBlocks;   // scan entries: blocks, or (sharded) rows
    // the list block lo of this lane's position j (the wave's positions: `need`)
    auto find_lo = [&](const int j, const bool fromList, const unsigned long long need) __attribute__((always_inline)) {
        const int jA = __builtin_amdgcn_readlane(j, (int)__builtin_ctzll(need));
        const int jB = __builtin_amdgcn_readlane(j, 63 - (int)__builtin_clzll(need));
        int lo = 0;
        if (jB - jA <= 1) {
            const int jj = (lane < 32) ? jA : jB;
            const int sub = lane & 31;
            int idx = sub * 32;
            unsigned long long m = __ballot((idx < nS ? sPfx[idx] : INT_MAX) <= jj);
            const int cA = __popcll(m & 0xffffffffull) - 1, cB = __popcll(m >> 32) - 1;
            idx = ((lane < 32) ? cA : cB) * 32 + sub;
            m = __ballot((idx < nS ? sPfx[idx] : INT_MAX) <= jj);
            lo = (j == jA) ? cA * 32 + __popcll(m & 0xffffffffull) - 1 : cB * 32 + __popcll(m >> 32) - 1;
        } else {
            // k < 64: the wave's positions jA .. jB are consecutive and span a couple of
            // blocks (a block holds A / nBlocks > 4 of them on average), so the block of jA
            // by the same 32-ary ballot search, then each lane steps forward (was a
            // 10-step binary search per lane: iterations 2-10 of the c3 window)
            const int sub = lane & 31;
            int idx = sub * 32;
            unsigned long long m = __ballot((idx < nS ? sPfx[idx] : INT_MAX) <= jA);
            const int c = __popcll(m & 0xffffffffull) - 1;
            idx = c * 32 + sub;
            m = __ballot((idx < nS ? sPfx[idx] : INT_MAX) <= jA);
            lo = c * 32 + __popcll(m & 0xffffffffull) - 1;
            if (fromList)
                while (lo + 1 < nS && sPfx[lo + 1] <= j) ++lo;
        }
        return lo;
    };
    if (need) {
        const int lo = find_lo(j, fromList, need);
#if SBMP_VALU_DUP == 2   // diagnostics (VALU by part): the search once more, on opaque copies
        {
            int j2 = j;
            asm volatile("" : "+v"(j2));
            asm volatile("" ::"v"(find_lo(j2, fromList, need)));
        }
#endif
        if (fromList) {
            if constexpr (SH) {   // the row's blocks: from the LDS table (round 4: one more L2 round trip)
                int blk, idx;
                row_locate_any(d, sv, sC16, lo, j - sPfx[lo], &blk, &idx);
                src = list_entry<SH>(d, pp, blk, idx);
            } else {
                src = list_entry<SH>(d, pp, lo, j - sPfx[lo]);
            }
            srcCost = reinterpret_cast<const SBMP_GAS float*>(src + 2);
        }
    }
#ifdef SBMP_TL_PROLOGUE   // stamp 5 = parent located (instead of the epilogue barrier)
    SBMP_STAMP(5);
#endif
    // Parent and obstacles are issued back to back and waited for together.
    float4 p;
    float parentCost;
    if (SH && fromList && !d.listPlain) {   // the owner's list over the mapping: system-scope loads
        p = load_record_g(src);
        parentCost = load_record_g(src + 2).x;
    } else {
        p = *src;
        parentCost = *srcCost;
    }
    float4 ro[kRegObs > 0 ? kRegObs : 1];
#pragma unroll
    for (int i = 0; i < kRegObs; ++i) ro[i] = G(d.obstacles)[i];
    insert_prev();
    if (kLdsObs) {
        if (tid < d.nObs) sObs[tid] = obsReg;
        for (int i = tid + kBlock; i < d.nObs; i += kBlock) sObs[i] = G(d.obstacles)[i];
        __syncthreads();
    }
    // the grid index's cell-start table into LDS: every row lookup of the Euler loop is
    // then an LDS read instead of an L2 round trip (the boxes stay in global memory)
    int* const sGridStart =
        SH ? reinterpret_cast<int*>(sC16 + (d.c16Lds ? ((d.nBlocks + 7) & ~7) : 0)) : reinterpret_cast<int*>(sNew + nW);
    if constexpr (OBS == kObsGrid) {
        const int nStart = d.gridG * d.gridG + 1;
        const SBMP_GAS int* const gs = G(d.gridStart);
        for (int i = tid; i < nStart; i += 4 * kBlock) {
            int v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (i + u * kBlock < nStart) ? gs[i + u * kBlock] : 0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + u * kBlock < nStart) sGridStart[i + u * kBlock] = v[u];
        }
        __syncthreads();
    }
    SBMP_STAMP(2);
    const float4* obs = (kRegObs > 0) ? ro : kLdsObs ? sObs : d.obstacles;
    ChildOut out;
    bool valid = false;
    // The fast loop runs on every lane, outside any divergent branch, so its lane masks
    // need no merging with exec: inactive lanes (slots >= S) propagate row 0 with
    // controls from their unused stream, and their result is dropped.
    bool fast = false;
    if constexpr (AGENT == 0 && kRegObs > 0) {
        fast = car_fast_ok(d);   // per plan (uniform)
        if (fast) {
#if SBMP_VALU_DUP == 3   // diagnostics: the schedule and the theta bound once more, on opaque copies
            {
                float4 p2 = p;
                asm volatile("" : "+v"(p2.x), "+v"(p2.y), "+v"(p2.z), "+v"(p2.w));
                const StepSched s2 = car_schedule<OBS>(p2, parent, act, d, oLane);
                const unsigned long long tb = __ballot(!car_theta_bounded(p2, ctl, d));
                asm volatile("" ::"s"(s2.boxes), "s"(s2.bounds), "s"(tb));
            }
#endif
            valid = car_propagate_fast<OBS>(p, parent, act, ctl, d, obs, oLane, out);
        }
    }
    if (!fast) {
        out = ChildOut{};   // inactive lanes: defined values (the fast loop writes every lane)
        if (act)
            valid = (AGENT == 0) ? car_euler<OBS, OBS == kObsGrid>(p, ctl, d, obs, out, sGridStart)
                                 : point_euler<OBS, OBS == kObsGrid>(p, ctl, d, obs, out, sGridStart);
    }
    SBMP_STAMP(3);

    // ---- bins (KGMT.cu:390-391) and the accept test (KGMT.cu:394-411, D2)
    int q1 = -1, q2 = -1;
    if (act) bins_k(out.state.x, out.state.y, d, &q1, &q2);   // N = 16 (KGMT.cu:8)
#if SBMP_VALU_DUP == 4   // diagnostics: the binning once more, on opaque copies
    if (act) {
        float x2 = out.state.x, y2 = out.state.y;
        asm volatile("" : "+v"(x2), "+v"(y2));
        int a2, b2;
        bins_k(x2, y2, d, &a2, &b2);
        asm volatile("" ::"v"(a2), "v"(b2));
    }
#endif
    // The planner workgroup publishes iteration t's scores and snapshot as 8-B words
    // tagged with t (step_planner); each lane that takes the test reads its two words
    // from L2 now, and the stores below overlap that round trip.  q2 >= 0 implies q1 >= 0.
    const bool look = act && valid && q2 >= 0;
    unsigned long long sw = 0ull, aw = 0ull;
    if (look) {
        // Plain loads (the first try; agent-scope loads measured 0.1-0.3 us slower per
        // launch): the first wave of an XCD to load a line after the planner published
        // brings it into that XCD's L2 and later waves hit there instead of each going
        // to memory; a line loaded before publication carries an older tag, and the
        // re-read below (agent scope, past this CU's caches) corrects it.
        // (relaxed atomic loads at workgroup scope: the same plain, cacheable global_load,
        // without the data race a plain load of a word another workgroup stores would be)
        sw = __hip_atomic_load(pubCur + q1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        aw = __hip_atomic_load(pubCur + d.nR1 + (q2 >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    float u = 0.0f;
    if (valid) u = xorwow_uniform(rs);   // KGMT.cu:395 (valid implies act)
    // this slot's child (state, ctrl); meaningless on inactive lanes, which store nothing
    // (a stale flag past S re-reads its child below)
    float4 cs = out.state;
    float4 cc = make_float4(out.a, out.steer, out.dur, __int_as_float(parent));
    float cost = parentCost + out.dur;   // getCost (KGMT.cu:631-633), as the insert computes it
    if (act) {
        store_wt(d.uState, slot, cs);   // write-through: fewer dirty lines at the boundary
        store_wt(d.uCtrl, slot, cc);
        store_wt(d.rngA, slot, make_uint4(rs.v0, rs.v1, rs.v2, rs.v3));
        store_wt(d.rngB, slot, make_uint2(rs.v4, rs.d));
        if (q1 >= 0) atomicAdd(&sR1P[q1], valid ? 1 : 0x10000);
        if (d.r2log) {
            store_wt(d.r2log, (t % kFoldEvery) * d.logSlots + b * kBlock + tid, r2_key(q2, valid));
        } else if (q2 >= 0) {
            __hip_atomic_fetch_add(G(valid ? d.R2Valid : d.R2Invalid) + q2, 1, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    {   // tags must read t; a word read before the planner published it is re-read (bounded)
        const unsigned want = (unsigned)t;
        bool stale = look && (((unsigned)(sw >> 32) != want) | ((unsigned)(aw >> 32) != want));
        if (__ballot(stale) != 0ull) {
            const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
            for (;;) {
                __builtin_amdgcn_s_sleep(8);
                if (stale) {
                    sw = __hip_atomic_load(pubCur + q1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    aw = __hip_atomic_load(pubCur + d.nR1 + (q2 >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    stale = ((unsigned)(sw >> 32) != want) | ((unsigned)(aw >> 32) != want);
                }
                if (__ballot(stale) == 0ull) break;
                if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > kStepWaitTicks) {   // give up, report
                    if (stale)
                        __hip_atomic_exchange(&G(d.status)->error, kErrStepHandoff, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
    }
    bool accept = false;
    if (look) {   // accept_test (kgmt_rules.h), written out: as a call k_step's code changed
        const uint32_t bit = 1u << (q2 & 31);
        const bool r2Avail = (uint32_t)aw & bit;
        accept = (u <= __uint_as_float((uint32_t)sw)) || !r2Avail;
        if (!r2Avail) atomicOr(&sNew[q2 >> 5], bit);
    }
#ifndef SBMP_TL_PROLOGUE
    SBMP_STAMP(4);
#endif
    const unsigned long long mask = __ballot(accept);
    const unsigned long long word0 =   // lane 0's word
        ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(word >> 32), 0) << 32) |
        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)word, 0);
    const unsigned long long wordAll = word0 | mask;   // GNew |= accept (stale bits survive)
    const bool flagged = __builtin_amdgcn_inverse_ballot_w64(wordAll);   // this lane's bit of wordAll (a lane mask)
    if ((wordAll & ~__ballot(act)) != 0ull) {   // rare; keeps the wait below off the common path
        if (flagged && !act) {   // a stale flag on a slot past S: the child last written there
            cs = G(d.uState)[slot];
            cc = G(d.uCtrl)[slot];
            cost = G(d.treeCtrl)[__float_as_int(cc.w)].w + cc.z;
        }
    }
    bool inGoal = false;
    if (flagged && d.goalThreshold > 0.0f) {   // sqrtf(.) < r is false for every r <= 0 (and NaN)
        // in_goal (kgmt_rules.h), written out: as a call k_step's code changed
        const float dx = cs.x - d.goalX, dy = cs.y - d.goalY;
        inGoal = __builtin_sqrtf(dx * dx + dy * dy) < d.goalThreshold;
    }
    // index among the wave's flagged slots; the first goal child is the wave's lowest
    const int idxW = __builtin_amdgcn_mbcnt_hi((uint32_t)(wordAll >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wordAll, 0u));
    const int glW = first_lane_value(flagged && inGoal, idxW, kNoGoalIdx);
    if (lane == 0) {
        store_wt(d.gnewOut, slot >> 6, wordAll);
        sWaveCnt[wave] = __popcll(wordAll);
        sWaveGoal[wave] = glW;
    }
    __syncthreads();
#ifndef SBMP_TL_PROLOGUE
    SBMP_STAMP(5);
#endif
    const int c0 = sWaveCnt[0], c1 = sWaveCnt[1], c2 = sWaveCnt[2], c3 = sWaveCnt[3];
    const int waveOff = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
    if (flagged) {
        if constexpr (SH) {   // this rank's list of owned block b
            SBMP_GAS float4* e = G(d.recOut) + ((size_t)cp * d.recCap + (size_t)b * kBlock + waveOff + idxW) * kStepEntry;
            if (d.stepMirror) {   // into every rank's list mirror (global block gb), over xGMI for peers
                const size_t m = ((size_t)cp * d.nBlocks * kBlock + (size_t)gb * kBlock + waveOff + idxW) * kStepEntry;
                for (int q = 0; q < sv.nranks; ++q) {
                    SBMP_GAS float4* mq = G(d.mirrorPeer[q]) + m;
                    store_record_g(mq, cs);
                    store_record_g(mq + 1, cc);
                    store_record_g(mq + 2, make_float4(cost, 0.0f, 0.0f, 0.0f));
                }
            } else if (d.listPlain) {   // read on this GPU after this launch (a local group)
                e[0] = cs;
                e[1] = cc;
                e[2] = make_float4(cost, 0.0f, 0.0f, 0.0f);
            } else {             // read by the peers over the mapping: written through
                store_record_g(e, cs);
                store_record_g(e + 1, cc);
                store_record_g(e + 2, make_float4(cost, 0.0f, 0.0f, 0.0f));
            }
        } else {
#ifdef SBMP_SOFFSET_DEMO   // the round-3 form of these stores (kgmt_device.h, SBMP_WT_OFF)
            const __amdgpu_buffer_rsrc_t rl = wt_rsrc(d.stepList);
            const int so = __builtin_amdgcn_readfirstlane(((cp * d.nBlocks + b) * kBlock) * kStepEntry * 16);
            const int vo = (waveOff + idxW) * kStepEntry * 16;
            __builtin_amdgcn_raw_buffer_store_b128(sbmp_u32x4{__float_as_uint(cs.x), __float_as_uint(cs.y), __float_as_uint(cs.z), __float_as_uint(cs.w)}, rl, vo, so, 0);
            __builtin_amdgcn_raw_buffer_store_b128(sbmp_u32x4{__float_as_uint(cc.x), __float_as_uint(cc.y), __float_as_uint(cc.z), __float_as_uint(cc.w)}, rl, vo + 16, so, 0);
            __builtin_amdgcn_raw_buffer_store_b128(sbmp_u32x4{__float_as_uint(cost), 0u, 0u, 0u}, rl, vo + 32, so, 0);
#else
            // < 2^27 entries; the row part is uniform, the lane part a 24-bit multiply (full rate)
            const int e = (cp * d.nBlocks + b) * kBlock * kStepEntry + (int)__umul24((unsigned)(waveOff + idxW), (unsigned)kStepEntry);
            store_wt(d.stepList, e, cs);
            store_wt(d.stepList, e + 1, cc);
            store_wt(d.stepList, e + 2, make_float4(cost, 0.0f, 0.0f, 0.0f));
#endif
        }
    }
    {   // one 64-bit atomic per touched cell, into this workgroup's replica
        SBMP_GAS unsigned long long* const rep =
            (SH ? G(d.stepXs[cp]) : G(d.stepDelta) + (size_t)(t % 3) * kDeltaReps * d.nR1) + (size_t)(b % kDeltaReps) * d.nR1;
        const int v = sR1P[tid];   // nR1 == kBlock
        if (v)
            __hip_atomic_fetch_add(rep + tid, r1_delta_word(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (SH) {   // R2New as bytes of the exchange (a sum over ranks), one store per cell the block saw
        SBMP_GAS uint8_t* const nb = reinterpret_cast<SBMP_GAS uint8_t*>(G(d.stepXs[cp]) + d.xNewOff);
        for (int i = tid; i < nW; i += kBlock) {
            uint32_t w = sNew[i];
            while (w) {   // written through (sc1): the fused exchange reads them in this launch
                __hip_atomic_store(nb + 32 * i + __builtin_ctz(w), (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                w &= w - 1u;
            }
        }
    } else {
        // replicas: a device atomic on one word serialises (~11 ns each); in the early
        // iterations most blocks set the same few words, so each replica sees 1/kNewReps
        SBMP_GAS uint32_t* const newCur = G(d.stepR2New) + ((size_t)(t % 3) * kNewReps + (size_t)(b % kNewReps)) * nW;
        if (nW <= 2 * kBlock) {   // n <= 8 (uniform): both words' LDS reads, then their atomics
            const uint32_t w0 = tid < nW ? sNew[tid] : 0u, w1 = tid + kBlock < nW ? sNew[tid + kBlock] : 0u;
            if (w0) __hip_atomic_fetch_or(newCur + tid, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (w1) __hip_atomic_fetch_or(newCur + tid + kBlock, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            for (int i = tid; i < nW; i += kBlock) {
                const uint32_t w = sNew[i];
                if (w) __hip_atomic_fetch_or(newCur + i, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (tid == 0) {   // the block's flagged count and its lowest goal child (in-block index)
        const int g0 = sWaveGoal[0], g1 = sWaveGoal[1], g2 = sWaveGoal[2], g3 = sWaveGoal[3];
        const int gmin = lowest_goal(c0, c1, c2, g0, g1, g2, g3);
        const int cw = (c0 + c1 + c2 + c3) | ((gmin == kNoGoalIdx ? 0 : gmin + 1) << 16);
        if constexpr (SH) {   // the block word, and this rank's part of row b (the exchange sums the row); sc1
            __hip_atomic_store(reinterpret_cast<SBMP_GAS int*>(G(d.stepXs[cp]) + d.xCntOff) + gb, cw, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(reinterpret_cast<SBMP_GAS int*>(G(d.stepXs[cp]) + d.xRowOff) + b,
                               (c0 + c1 + c2 + c3) | ((gmin == kNoGoalIdx ? 0 : 1) << 16), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            // the count again as u16 (the summed exchange forms carry it; the compact one rebuilds it)
            store_wt(reinterpret_cast<uint16_t*>(d.stepXs[cp] + d.xC16Off), gb, (uint16_t)(c0 + c1 + c2 + c3));
        }
        else store_wt(d.stepCnt, cp * kMaxStepBlocks + b, cw);
    }
    SBMP_STAMP(6);
    if (tl) stamp[7] = placement_stamp();
    if (tl && lane == 0)
        for (int i = 0; i < kTimelineStamps; ++i) G(tl)[i] = stamp[i];
    };
    body();
    fx_exit();
#undef SBMP_STAMP

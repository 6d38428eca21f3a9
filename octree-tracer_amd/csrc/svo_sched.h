// svo_sched.h -- the strip schedule's per-frame policy: which lists a STACK frame is traced with, and
// what the post pass measures and rebuilds after it.  Plain C++ (no HIP): the host glue in svo_abi.cpp (trace_launch) measures the
// facts and runs the launches, tests/test_schedule_plan.py replays frame sequences through these two functions.  Also the arithmetic
// of the trace kernel's strip claims (which entry of which list a wave gets), stated once for the kernel and for a host test.  And
// which kernel traces a frame, with how many workgroups (TraceChoice, trace_slot, resident_workgroups, stack_grid_blocks): the one
// statement of those rules, for svo_abi.cpp, for svo_kernels.hip's launcher and for tests/test_trace_choice_host.py.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace svo {

// Frames of a resting view whose list times are fed back into the shares: the lists are rebuilt after each of them, and the last
// one puts back the best shares seen since the layout was new (svo_kernels.hip: balance_step).
constexpr uint32_t kBalanceLearnFrames = 16;
// a schedule that has not been rebuilt for this many frames is no longer taken for the same input (a backstop for node buffers
// written behind the context's back)
constexpr uint32_t kSchedMaxAge = 64;

// What a schedule slot remembers between frames (its device buffers and the inputs it was built from live in svo_ctx::Sched).
struct SchedState {
    bool valid = false;           // costs and lists belong to the current work layout (same pixels behind every strip)
    bool order_filtered = false;  // the lists were built for one frame without its empty / culled strips: not a general schedule
    uint32_t age = 0;             // frames since the last rebuild
    uint32_t balance_frames = 0;  // scheduled frames of this layout whose stamps have been fed back
    bool floored = false;         // the lists were built with the motion floor (then they are rebuilt once more, exactly, at rest)
};

// What the caller measures for a STACK frame.
struct FrameFacts {
    bool schedule = false;     // scheduling is on and the frame has no more than kMaxScheduledStrips strips
    bool filtered = false;     // this frame's lists are built before the trace without the strips that hold no ray (skip mask, culling)
    bool same_layout = false;  // the work layout is the one the slot's costs were measured on
    bool same_input = false;   // camera and tree are the ones the lists were built from (caller-supplied rays: never)
    bool moving = false;       // the camera differs from the previous frame's
    uint32_t mode = 0, n_rects = 0;  // of the WorkDesc
    uint32_t motion_floor = 0;       // SVO_OPT_SCHEDULE_MOTION (0: off)
    uint32_t sched_period = 1;       // frames between rebuilds while the input moves
    bool balance = false;            // list-share feedback on (SVO_NO_LIST_BALANCE unset)
};

struct TracePlan {
    bool reset_shares = false;  // a new layout starts from equal shares of the lists
    bool feed_balance = false;  // the trace stamps the lists' times into the balance words
    bool stored_lists = false;  // trace from the complete lists built after an earlier frame
    bool prior_costs = false;   // filtered lists: ordered by the costs of an earlier frame (else screen order)
};

struct PostPlan {
    bool rebuild = false;      // the slot's costs are this frame's: measured by the post pass, or reused (reuse_costs)
    bool reuse_costs = false;  // a resting view rebuilt for the shares' sake only: its strips' cost classes are the ones measured last time
    bool build_lists = false;  // the post pass builds complete lists for the next frames (a filtered frame built its own before the trace)
    uint32_t motion_floor = 0;     // non-zero: strips near the long ones of this frame are not scheduled as cheap (strip_danger_kernel)
    uint32_t balance_update = 0;   // n > 0: the n-th frame fed back steps the shares (balance_step)
};

// list-share feedback of a schedule (balance_step): [0..8] cumulative shares of the 8 lists (16-bit fractions, [0] = 0, [8] = 65536),
// then the words below; behind them (kBalanceHead) one end stamp per workgroup of the trace launch (workgroup b started on list b % 8)
constexpr uint32_t kBalanceStart = 9;         // start stamp of the last frame's first workgroup
constexpr uint32_t kBalanceUpdates = 18;      // updates so far
constexpr uint32_t kBalanceStamps = 19;       // the last trace launch's workgroups
constexpr uint32_t kBalanceBestTime = 20;     // the shortest frame so far (ticks; 0: none yet)
constexpr uint32_t kBalanceBestShares = 21;   // [21..29] the shares it was traced with
constexpr uint32_t kBalanceHead = 32, kBalanceSlots = 4096, kBalanceWords = kBalanceHead + kBalanceSlots;
// a list's share of a cost class stays within these factors of an eighth, and moves by at most kShareStepMax per update
constexpr float kShareMin = 0.6f, kShareMax = 1.6f, kShareStepMin = 0.8f, kShareStepMax = 1.25f;

#if defined(__HIPCC__)
#define SVO_SCHED_HD __host__ __device__
#else
#define SVO_SCHED_HD
#endif

// The share step of one fed-back frame, after its stamps are reduced (svo_kernels.hip: balance_step, one thread; tests/test_sched_host.py
// drives it on the host).  T[k]: the mean time of list k's sampled workgroups (0: none of them left a stamp), t_last: the latest
// stamp (the frame's time; 0: none), update: n = the n-th frame fed back, bal: the kBalanceHead head words.
// Keep-best: the shares the frame was traced with are noted when it beat every frame since the layout was new; update
// kBalanceLearnFrames puts the best ones back and steps no more.  Otherwise share *= 1 + gain (mean / T - 1), the ratio clamped to
// kShareStepMin .. kShareStepMax and the share to kShareMin .. kShareMax eighths, and the eight are renormalised to cumulative 16-bit
// fractions.  No step when a list has no stamp.
// After it bal[0] = 0 < bal[1] < ... < bal[8] = 65536 and no share exceeds a quarter (16384), which is what order_list_cap relies on.
// By induction from the equal shares: a share leaves the clamp at no more than kShareMax / 8 = 13107.2, while the other seven sum to
// at least 65536 - 16384 = 49152 before the step.  A step takes gain * (1 - kShareStepMin) = 12 % of a share at the largest gain
// (0.6), and the upper clamp takes more only from a share above 13107.2 / 0.88 = 14894.  No share is ever below 3072 (the lower
// clamp, 4915.2, of a sum of at most 8 * 13107.2), so the seven lose most when they are 16384, 16384, 4096 and four times 3072:
// they keep 2 * 13107.2 + 0.88 * 16384 = 40632, and the renormalised share is at most 13107.2 / (13107.2 + 40632) = 0.2439,
// 15984 of 65536 -- 400 below 16384, where rounding the cumulative fractions adds at most one.  Lists that stay fastest settle
// near 0.227 (tests/test_sched_host.py holds every update to the bound).
SVO_SCHED_HD inline void balance_share_step(uint32_t *bal, const float T[8], uint32_t t_last, float gain, uint32_t update) {
    if (update <= kBalanceLearnFrames && t_last != 0u && (update == 1u || bal[kBalanceBestTime] == 0u || t_last < bal[kBalanceBestTime])) {
        bal[kBalanceBestTime] = t_last;
        for (int k = 0; k <= 8; k++) bal[kBalanceBestShares + k] = bal[k];
    }
    if (update == kBalanceLearnFrames && bal[kBalanceBestTime] != 0u) {  // the schedule built next is the one a resting view keeps
        for (int k = 0; k <= 8; k++) bal[k] = bal[kBalanceBestShares + k];
        bal[kBalanceUpdates] += 1u;
        return;
    }
    float w[8], mean = 0.0f;
    for (int k = 0; k < 8; k++) {
        if (!(T[k] > 0.0f)) return;
        w[k] = (float)(bal[k + 1] - bal[k]);
        mean += T[k] * 0.125f;
    }
    float sum = 0.0f;
    for (int k = 0; k < 8; k++) {
        const float r = fminf(fmaxf(mean / T[k], kShareStepMin), kShareStepMax);
        w[k] = fminf(fmaxf(w[k] * (1.0f + gain * (r - 1.0f)), kShareMin * 8192.0f), kShareMax * 8192.0f);
        sum += w[k];
    }
    uint32_t acc = 0u;
    float run = 0.0f;
    for (int k = 0; k < 8; k++) {
        bal[k] = acc;
        run += w[k];
        acc = k == 7 ? 65536u : (uint32_t)(run / sum * 65536.0f + 0.5f);
    }
    bal[8] = 65536u;
    bal[kBalanceUpdates] += 1u;
}

// ---- strip claims: which entry of which list a wave of the trace kernel gets (svo_kernels.hip: trace_stack_body and its entry_of; tests/test_claims_host.py
// holds these functions to each other) ----
// A frame's strips stand in kShards lists, one per XCD.  The first entries of a list are RESERVED, one per wave that starts on
// it; behind them each of the list's kSubs claim counters hands out every kSubs-th entry.
// (inlined before anything is simplified: the trace kernel's claim code is then compiled as if it were written out in place)
#define SVO_SCHED_INLINE inline __attribute__((always_inline))
constexpr uint32_t kShards = 8, kSubs = 8;
constexpr uint32_t kDealRun = 16;            // the no-schedule deal: consecutive strips that go to one list
constexpr uint32_t kNoStrip = 0xFFFFFFFFu;   // "past the end of the list"

// Waves that start on list l in a grid of `blocks` workgroups of `waves_per_block` waves (workgroup b starts on list b % kShards):
// the list's reserved entries.
SVO_SCHED_HD SVO_SCHED_INLINE uint32_t waves_starting_on(uint32_t l, uint32_t blocks, uint32_t waves_per_block) {
    return ((blocks + kShards - 1u - l) / kShards) * waves_per_block;
}
// Where a wave starts: workgroup b on list b % kShards, its wave w with the reserved entry of its rank among the list's waves, and
// with the list's counter (b / kShards) % kSubs -- as one number, list * kSubs + counter, the way the kernel keeps it.
SVO_SCHED_HD SVO_SCHED_INLINE uint32_t starting_rank(uint32_t b, uint32_t w, uint32_t waves_per_block) { return (b / kShards) * waves_per_block + w; }
SVO_SCHED_HD SVO_SCHED_INLINE uint32_t starting_counter(uint32_t b) { return (b % kShards) * kSubs + (b / kShards) % kSubs; }
// The list entry that the k-th answer of a list's counter j stands for.
SVO_SCHED_HD SVO_SCHED_INLINE uint32_t claimed_entry(uint32_t k, uint32_t j, uint32_t reserved) { return k * kSubs + j + reserved; }
// The stealing probe's question: has counter j of a list of `len` entries, read as cv, an entry left to hand out?
SVO_SCHED_HD SVO_SCHED_INLINE bool counter_has_entry(uint32_t cv, uint32_t j, uint32_t reserved, uint32_t len) {
    return (uint64_t)cv * kSubs + j + reserved < (uint64_t)len;
}
// No schedule yet (the first frame of a layout): runs of kDealRun consecutive strips dealt round-robin to the lists, so that the
// lists are equally long in work whatever part of the screen is expensive (8 contiguous regions left whole lists of sky idle
// early and their waves stealing, one probe and one synchronous claim per strip).
// The strip behind entry k of list l (kNoStrip: past the end) ...
SVO_SCHED_HD SVO_SCHED_INLINE uint32_t dealt_strip(uint32_t l, uint32_t k, uint32_t n_strips) {
    const uint32_t cand = ((k / kDealRun) * kShards + l) * kDealRun + k % kDealRun;
    return cand < n_strips ? cand : kNoStrip;
}
// ... where a strip stands ...
SVO_SCHED_HD SVO_SCHED_INLINE void dealt_place(uint32_t strip, uint32_t &l, uint32_t &k) {
    const uint32_t run = strip / kDealRun;
    l = run % kShards;
    k = (run / kShards) * kDealRun + strip % kDealRun;
}
// ... and how long list l is: run g belongs to list g mod kShards, and the last run may be short.
SVO_SCHED_HD SVO_SCHED_INLINE uint32_t dealt_length(uint32_t l, uint32_t n_strips) {
    const uint32_t runs = (n_strips + kDealRun - 1u) / kDealRun, mine = runs > l ? (runs - l + kShards - 1u) / kShards : 0u;
    return mine * kDealRun - ((runs != 0u && (runs - 1u) % kShards == l) ? runs * kDealRun - n_strips : 0u);
}

inline bool stored_lists(const SchedState &s) { return s.valid && !s.order_filtered; }

inline TracePlan plan_before_trace(SchedState &s, const FrameFacts &f) {
    TracePlan p;
    if (!f.schedule) return p;
    if (!f.same_layout) s.valid = false;
    p.reset_shares = !s.valid;
    if (p.reset_shares) s.balance_frames = 0;
    p.feed_balance = f.balance;
    p.prior_costs = f.filtered && s.valid;
    if (f.filtered) s.order_filtered = true;  // these lists leave strips out: good for this frame only
    p.stored_lists = !f.filtered && stored_lists(s);
    return p;
}

// Rebuild the schedule when there is none, and every sched_period frames while the input moves.  A ray's step count does not
// depend on the order it was traced in, so a schedule measured on this camera and tree stays exact as long as both stay put.
inline PostPlan plan_after_trace(SchedState &s, const FrameFacts &f) {
    const bool same_input = f.same_input && s.age < kSchedMaxAge;
    // a frame traced with complete lists also feeds the time its lists took back into their shares: while camera and tree stay put
    // the lists are rebuilt for the first kBalanceLearnFrames such frames, then the shares have settled
    const bool fed_back = f.schedule && f.balance && !f.filtered && stored_lists(s);
    const bool learning = same_input && fed_back && s.balance_frames < kBalanceLearnFrames;
    const bool complete_again = s.order_filtered && !f.filtered;  // the stored lists leave strips out: complete ones are built now
    const bool at_rest_floored = same_input && s.floored && !f.moving;  // the exact rebuild after floored motion
    const bool due = !same_input && s.age + 1 >= f.sched_period;
    PostPlan p;
    p.rebuild = f.schedule && (!s.valid || complete_again || due || at_rest_floored || learning);
    p.reuse_costs = p.rebuild && s.valid && learning && !complete_again && !at_rest_floored;
    p.build_lists = p.rebuild && !f.filtered;
    const bool floor = p.build_lists && f.moving && f.motion_floor != 0u && f.mode == 0u && f.n_rects == 1u;
    p.motion_floor = floor ? f.motion_floor : 0u;
    p.balance_update = fed_back && (!same_input || s.balance_frames < kBalanceLearnFrames) ? s.balance_frames + 1u : 0u;
    if (fed_back) s.balance_frames++;
    if (p.build_lists) {
        s.floored = floor;
        s.order_filtered = false;
    }
    if (p.rebuild) {
        s.valid = true;
        s.age = 0;
    } else if (f.schedule) {
        s.age++;
    }
    return p;
}

// ---- the trace kernel of a frame and its grid: svo_abi.cpp asks (trace_launch and the callers that allocate by the answer),
// svo_kernels.hip launches what it is told (plan_trace, launch_trace); tests/test_trace_choice_host.py holds both to a restatement ----
constexpr int kTopLevels = 3;         // K: octree levels folded into the LDS top table
constexpr int kStackBlock = 256;      // threads of a STACK workgroup
constexpr int kStackLevels = 12;      // default: resolves levels up to 3 + 1 + 12 = 16
constexpr int kStackLevelsDeep = 18;  // deep trees: up to level 22 = kPathBits - 1
constexpr int stack_max_depth(bool deep) { return kTopLevels + 1 + (deep ? kStackLevelsDeep : kStackLevels); }
constexpr uint32_t kTimelineWaves = 16384;  // SVO_DEBUG_WAVES of include/svo_hip.h (svo_device.h holds the two to each other)

// What the host knows before it traces a call's frames (the uniforms' flags as they are set; the options as the caller left them).
struct TraceFacts {
    bool restart_variant = false;  // SVO_OPT_VARIANT is SVO_VARIANT_RESTART
    uint32_t tree_depth = 16;      // SVO_OPT_TREE_DEPTH: the caller's bound on the octree's depth
    bool pause_adaptive = false, show_hits = false, misc_bool = false;  // SVO_F_*
    bool fused_shadows = false;    // SVO_OPT_FUSED_SHADOWS is not 0
};
// ... and of one launch
struct LaunchFacts {
    uint32_t mode = 0;          // of the WorkDesc
    bool count_rays = false;    // explicit rays that count like primary ones (shadow and secondary rays)
    bool fused = false;         // the caller fused the shadow rays (fuse_allowed, and its own test of the sun's direction)
    bool debug_buffer = false;  // SVO_OPT_DEBUG_BUFFER is set
};

// What runs.  RESTART: the reference-shaped walk, general to depth 31; of the fields below only cnt means something (the hit
// counters are live).  STACK: trace_stack_kernel<.., ge, dbg, cnt, shd> with the default or the deep ancestor stack, or the
// replay twin of the plain default one.
struct TraceChoice {
    bool stack = false;
    bool ge = false;      // SVO_F_MISC_BOOL: the hit test is >=
    bool deep = false;    // 19-level ancestor stack (trees deeper than 16 levels): more LDS per workgroup, fewer resident waves
    bool dbg = false;     // the timeline build
    bool cnt = false;     // hit counters live
    bool shd = false;     // fused shadow rays
    bool replay = false;  // a resting view's static deal (svo_deal.h): no claims
};

// The debug view that reads counter bits needs the reference-shaped walk: RESTART, and nothing fused into it.
inline bool debug_view(const TraceFacts &f) { return f.pause_adaptive && f.show_hits; }
// STACK resolves the levels its integer path codes cover; deeper trees take the general RESTART kernel.  (Wanted is not chosen:
// the debug view has its top table built and is then traced by RESTART.)
// The ancestor stack's levels for a tree of the declared depth (0: deeper than either stack resolves).
inline int stack_levels_for(uint32_t tree_depth) {
    if (tree_depth <= (uint32_t)stack_max_depth(false)) return kStackLevels;
    return tree_depth <= (uint32_t)stack_max_depth(true) ? kStackLevelsDeep : 0;
}
inline bool stack_wanted(const TraceFacts &f) { return !f.restart_variant && stack_levels_for(f.tree_depth) != 0; }
// The kind of kernel every launch of the call gets; the per-launch fields are launch_choice's.
inline TraceChoice kernel_kind(const TraceFacts &f) {
    TraceChoice c;
    c.stack = stack_wanted(f) && !debug_view(f);
    c.ge = f.misc_bool;
    c.deep = stack_levels_for(f.tree_depth) == kStackLevelsDeep;
    return c;
}
// May the primary launch trace the shadow rays too?  (The caller adds what only it can test: the sun's direction.)
inline bool fuse_allowed(const TraceFacts &f) { return f.fused_shadows && kernel_kind(f).stack; }
inline TraceChoice launch_choice(const TraceFacts &f, const LaunchFacts &l) {
    TraceChoice c = kernel_kind(f);
    // shader.wgsl:159: counters are live unless pause_adaptive; rays handed in by the caller (svo_trace_rays) never count
    c.cnt = (l.mode != 2u || l.count_rays) && !f.pause_adaptive;
    c.shd = c.stack && l.fused;
    c.dbg = c.stack && l.debug_buffer && !c.shd;  // (there is no timeline build with fused shadows)
    return c;
}
// The launches the replay kernel can serve (the rest of a plain static frame is the deal's own: svo_abi.cpp, deal_before).  With
// shd excluded, dbg says whether the debug buffer is set.
inline bool replay_eligible(const TraceChoice &c) { return c.stack && !c.cnt && !c.shd && !c.dbg && !c.deep; }

// One slot per STACK instantiation, for the table of kernels and the context's cache of resident workgroups per CU.  The
// replay twin has the slot of the default instantiation whose claims it replaces: same grid, same LDS.
constexpr uint32_t kTraceSlots = 24;
inline uint32_t trace_slot(const TraceChoice &c) {
    const uint32_t kind = c.shd ? 4u + c.cnt : 2u * c.dbg + c.cnt;
    return (c.ge ? 12u : 0u) + (c.deep ? 6u : 0u) + kind;
}

// Resident workgroups per CU of a kernel that asks for lds_bytes per workgroup, from the runtime's answer.
// The occupancy query does not round LDS up to the allocation granule; measured on MI355X, 336 bytes on top of
// 26 KiB per workgroup already cost the sixth workgroup per CU.  Workgroups that are not resident at launch
// start when the first ones end and bring their reserved (longest) strips with them, so overestimating is
// far worse than underestimating.  The granule is 1280 bytes (320 dwords): 512 bytes on top of the default kernel's 22 KiB keep the
// seventh workgroup per CU, 528 lose it (profiles/r04_lds_granule_ab.log).
inline int resident_workgroups(int by_runtime, size_t lds_bytes) {
    const int n = by_runtime > 0 ? by_runtime : 1;
    const size_t granules = (lds_bytes + 1279u) / 1280u;
    const int by_lds = granules ? (int)((160u * 1024u) / (granules * 1280u)) : 0;
    return by_lds >= 1 && by_lds < n ? by_lds : n;
}
// Workgroups of a STACK launch: every CU full (or SVO_OPT_GRID_BLOCKS, when not 0), and no more than the frame has strips for
// its waves.
inline uint32_t stack_grid_blocks(uint32_t num_cus, uint32_t resident_per_cu, uint32_t grid_override, bool debug_buffer, uint32_t n_items,
                                  uint32_t strip_items) {
    constexpr uint32_t waves = kStackBlock / 64;
    uint32_t blocks = num_cus * resident_per_cu;
    if (grid_override > 0u) blocks = grid_override;
    // (the timeline's buffer has a row for kTimelineWaves waves: a grid override beyond that is cut back while the buffer is set,
    // also for the fused kernel, which writes no timeline)
    if (debug_buffer && blocks > kTimelineWaves / waves) blocks = kTimelineWaves / waves;
    const uint32_t n_strips = (n_items + strip_items - 1u) / strip_items;
    const uint32_t need = (n_strips + waves - 1u) / waves;
    return blocks > need ? need : blocks;
}

#undef SVO_SCHED_INLINE

}  // namespace svo

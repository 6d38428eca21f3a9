// svo_sched.h -- the strip schedule's per-frame policy: which lists a STACK frame is traced with, and
// what the post pass measures and rebuilds after it.  Plain C++ (no HIP): the host glue in svo_abi.cpp (trace_launch) measures the
// facts and runs the launches, tests/test_schedule_plan.py replays frame sequences through these two functions.
#pragma once
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

}  // namespace svo

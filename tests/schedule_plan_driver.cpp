// Replays frames through the strip schedule's policy (octree-tracer_amd/csrc/svo_sched.h) the way trace_launch does, with
// integers standing in for the uniforms, the node-store version and the work layout: one frame per input line (see
// tests/test_schedule_plan.py), one row per frame out:
//   frame | lists (L stored, F filtered, - none) reset_shares feed_balance prior_costs
//         | measure reuse_costs build_lists floor balance_update | valid order_filtered age balance_frames floored
#include <cstdio>

#include "svo_sched.h"

struct Slot {  // svo_ctx::Sched
    svo::SchedState state;
    int key = 0, built_cam = 0, built_ver = 0, prev_cam = 0;
    bool have_prev = false;
};

int main() {
    Slot slots[2];
    int cam, ver, layout, mode, slot, rects, filt, sched, floor, period, balance, grow;
    for (int frame = 0; scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &cam, &ver, &layout, &mode, &slot, &rects, &filt, &sched,
                              &floor, &period, &balance, &grow) == 12;
         frame++) {
        Slot &sc = slots[slot & 1];
        if (sched && grow) sc = Slot{};
        svo::FrameFacts f;
        f.schedule = sched;
        f.filtered = sched && filt;
        f.same_layout = sc.key == layout;
        f.mode = (uint32_t)mode;
        f.n_rects = (uint32_t)rects;
        f.motion_floor = (uint32_t)floor;
        f.sched_period = (uint32_t)period;
        f.balance = balance;
        const svo::TracePlan tp = svo::plan_before_trace(sc.state, f);
        f.same_input = (mode != 2 || slot == 1) && sc.built_ver == ver && sc.built_cam == cam;
        f.moving = sc.have_prev && sc.prev_cam != cam;
        const svo::PostPlan pp = svo::plan_after_trace(sc.state, f);
        sc.prev_cam = cam;
        sc.have_prev = true;
        if (pp.rebuild) {
            sc.key = layout;
            sc.built_cam = cam;
            sc.built_ver = ver;
        }
        const svo::SchedState &s = sc.state;
        printf("%3d | %s %d %d %d | %d %d %d %d %2u | %d %d %2u %2u %d\n", frame, f.filtered ? "F" : (tp.stored_lists ? "L" : "-"),
               tp.reset_shares, tp.feed_balance, tp.prior_costs, pp.rebuild && !pp.reuse_costs, pp.reuse_costs, pp.build_lists,
               pp.motion_floor != 0u, pp.balance_update, s.valid, s.order_filtered, s.age, s.balance_frames, s.floored);
    }
}

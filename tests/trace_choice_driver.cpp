// Prints what octree-tracer_amd/csrc/svo_sched.h says about the trace kernel of a frame and its grid, for
// tests/test_trace_choice_host.py to hold against a restatement.  One command per input line:
//   choice V D PA SH MB MODE CR FUSE DBG REPLAY
//                    variant (0 RESTART, 1 STACK), declared depth, the flags PAUSE_ADAPTIVE, SHOW_HITS and MISC_BOOL, the work mode,
//                    count_rays, SVO_OPT_FUSED_SHADOWS != 0 (the sun's direction is taken to pass the caller's test), debug buffer
//                    set, and whether the deal's plan asks for a replay -- put together the way svo_abi.cpp does it.
//                    "K wanted fuse | stack ge deep dbg cnt shd replay | slot"
//   slots            "N kTraceSlots", then per STACK instantiation "S ge deep dbg cnt shd slot" and per replay twin "R ge slot"
//   resident RT LDS  "B n": resident workgroups per CU when the runtime answers RT for a kernel with LDS bytes of LDS
//   grid CUS PER OVERRIDE DBG ITEMS STRIP
//                    "G blocks": the workgroups of a STACK launch
#include <cstdio>
#include <cstring>

#include "svo_sched.h"

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "choice")) {
            unsigned v, depth, pa, sh, mb, mode, cr, fuse, dbg, replay;
            if (scanf("%u %u %u %u %u %u %u %u %u %u", &v, &depth, &pa, &sh, &mb, &mode, &cr, &fuse, &dbg, &replay) != 10) return 1;
            svo::TraceFacts f;
            f.restart_variant = v == 0;
            f.tree_depth = depth;
            f.pause_adaptive = pa, f.show_hits = sh, f.misc_bool = mb;
            f.fused_shadows = fuse;
            svo::LaunchFacts l;
            l.mode = mode;
            l.count_rays = cr;
            l.fused = svo::fuse_allowed(f);
            l.debug_buffer = dbg;
            svo::TraceChoice c = svo::launch_choice(f, l);
            c.replay = replay && svo::replay_eligible(c);
            printf("K %d %d | %d %d %d %d %d %d %d | %u\n", (int)svo::stack_wanted(f), (int)l.fused, (int)c.stack, (int)c.ge, (int)c.deep,
                   (int)c.dbg, (int)c.cnt, (int)c.shd, (int)c.replay, svo::trace_slot(c));
        } else if (!strcmp(cmd, "slots")) {
            printf("N %u\n", svo::kTraceSlots);
            for (int bits = 0; bits < 32; bits++) {
                svo::TraceChoice c;
                c.stack = true;
                c.ge = bits & 16, c.deep = bits & 8, c.dbg = bits & 4, c.cnt = bits & 2, c.shd = bits & 1;
                if (c.dbg && c.shd) continue;  // (no such instantiation)
                printf("S %d %d %d %d %d %u\n", (int)c.ge, (int)c.deep, (int)c.dbg, (int)c.cnt, (int)c.shd, svo::trace_slot(c));
            }
            for (int ge = 0; ge < 2; ge++) {
                svo::TraceChoice c;
                c.stack = c.replay = true;
                c.ge = ge;
                printf("R %d %u\n", ge, svo::trace_slot(c));
            }
        } else if (!strcmp(cmd, "resident")) {
            int rt;
            unsigned lds;
            if (scanf("%d %u", &rt, &lds) != 2) return 1;
            printf("B %d\n", svo::resident_workgroups(rt, lds));
        } else if (!strcmp(cmd, "grid")) {
            unsigned cus, per, over, dbg, items, strip;
            if (scanf("%u %u %u %u %u %u", &cus, &per, &over, &dbg, &items, &strip) != 6) return 1;
            printf("G %u\n", svo::stack_grid_blocks(cus, per, over, dbg != 0, items, strip));
        } else {
            return 1;
        }
    }
}

// svo_device.h -- internal launch interface between the C ABI (svo_abi.cpp) and the gfx950
// kernels (svo_kernels.hip).  Not part of the public boundary (include/svo_hip.h).
// A trace is planned, then launched: svo_sched.h says which kernel a frame gets (TraceChoice) and how its grid is worked out,
// plan_trace turns a choice into a TraceLaunch for this device, launch_trace launches it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svo_hip.h"
#include "svo_sched.h"

namespace svo {

constexpr uint32_t kVoxelOffset = 134217728u;  // octree.rs:5
constexpr uint32_t kMaxDescent = 31;           // descent guard (see oracle/svo_oracle.c)
constexpr int kTopEntries = 1 << (3 * kTopLevels);
constexpr int kTopAuxEntries = 8 + 64;  // level-1 and level-2 cells -> child group of the next level (kTopLevels = 3)
constexpr int kPathBits = 23;                  // D: path-code bits per axis (grid units: 2^(D-1) per unit of the reference's cube, so that
                                               // 2^D + code is an exact f32 whose mantissa IS the code: DESIGN.md 4.2)
// Words between two claim counters.  Rounds 2 - 4 kept them 128 B apart (all 64 within 8 KB); round 5: 64 KB + 128 B apart.  Every claim is
// an atomic executed at the memory side, and while one is in flight the L2 channel it went through answers everything else more slowly
// (profiles/r05_pmc_claim_timing_ab.json) -- 8 KB of counters sit behind one or two channels, 4 MB of them behind all
// (profiles/r05_counter_stride_ab*.log: 1080p -1.1 / -3.4 %, 4K -1.6 / -0.3 % in two runs; 4 KB + 128 B: -0.5 / -2.5 %, -0.7 / -1.2 %)
#ifndef SVO_COUNTER_STRIDE
#define SVO_COUNTER_STRIDE 16416
#endif
constexpr int kCounterStride = SVO_COUNTER_STRIDE;
constexpr int kCounterWords = 64 * kCounterStride;  // 64 claim counters (8 lists x 8 counters)

// Top-table entry (one per level-K cell, index = cx << 2K | cy << K | cz): level << 27 | child group index.
// The level is K+1 below an interior cell, or the shallower level at which a leaf covers the whole cell
// (the descent then reads that leaf word itself).

// Work decomposition: a list of equally sized pixel rectangles, each cut into 64-pixel blocks (8x8 by default).
// Item q (one pixel slot): rect = q / (64 * blocks_per_rect); block and lane follow.
struct WorkDesc {
    uint32_t mode;        // 0: one rectangle at (x0, y0); 1: tiles first_tile + k * tile_stride; 2: explicit rays
    uint32_t x0, y0;      // mode 0 origin
    uint32_t w, h;        // rectangle size in pixels
    uint32_t bw_log2;     // pixel blocks are 2^bw_log2 wide and 64 / that high (8x8: 3)
    uint32_t bpr;         // blocks per rectangle row
    uint32_t bprect;      // blocks per rectangle
    uint32_t n_rects;
    uint32_t tiles_x;     // mode 1: tiles per frame row
    uint32_t first_tile, tile_stride;
    uint32_t n_items;     // mode 0/1: n_rects * bprect * 64; mode 2: n_rays
    uint32_t magic_bpr, magic_bprect, magic_tiles_x;  // floor(2^32 / d) + 1 (0 when d == 1), see fast_div
};

struct TraceArgs {
    const uint32_t *nodes;
    uint32_t n_words;
    const uint32_t *top_table;  // kTopEntries words (device) or nullptr
    svo_uniforms u;
    WorkDesc work;
    const float *rays;          // mode 2
    svo_hit *hits;              // may be nullptr
    uint32_t *rgba;             // may be nullptr
    float *aux_t;               // optional: t_current of the last step per record (the shading pass rebuilds HitInfo.pos)
    uint32_t *status;           // device word: bit 0 set when a STACK-variant descent exceeded kPathBits
    uint32_t refill_min;
    uint32_t cam_shortcut;      // STACK: 1 = rays that start at the camera's own position inside the cube share the wave's one first walk
    uint32_t *count_nodes;      // writable alias of nodes when hit counters are live (pause_adaptive off), else nullptr
    const uint32_t *order;      // STACK, optional: schedule built by strip_order_kernel (8 lengths + 8 lists)
    uint32_t order_cap;         // entries reserved per list
    uint32_t *debug;            // optional: 16 words per wave (start, queue-dry, end ticks of 10 ns, rounds, active-lane sum, ..., phase cycles)
    const uint8_t *skip;        // mode 2, optional: one byte per ray; non-zero = no ray here, its (all-zero) record is already written
    uint32_t *balance;          // STACK, optional: kBalanceWords words of the schedule's list-share feedback (see launch_post); the trace kernel
                                // records when its first wave started (kBalanceStart) and when a sample of every list's workgroups ended, 10 ns ticks
    svo_hit *shadow_hits;       // STACK, optional (fused shadow rays): the lane that finishes a primary ray with a hit goes on with that
                                // pixel's shadow ray (shader.wgsl:275-280) and writes its record here; pixels without one get zeros
    // STACK, optional (a resting view's static deal, svo_deal.h): non-null = the replay kernel traces this frame, wave w the strips of
    // row w of the table (deal_row_cap entries a row, 0xFFFFFFFF behind the last) and leaves two stamps in slot w of deal_stamps
    const uint32_t *deal_table;
    uint32_t deal_row_cap;
    uint32_t *deal_stamps;      // per wave: when it began its last strip, when it ended (10 ns ticks)
};

static_assert(kTimelineWaves == SVO_DEBUG_WAVES, "svo_sched.h caps the grid by the timeline buffer's rows");

struct LaunchInfo {
    int grid_blocks;         // 0 = auto
    int num_cus;
    int *occupancy;          // STACK: the context's cache of resident workgroups per CU, kTraceSlots of them (trace_slot)
    uint32_t strip_items;    // STACK: pixel slots a wave claims at a time (multiple of 64)
    uint32_t *counters;      // STACK: kCounterWords claim-counter words, zero when a frame starts
    uint32_t *defer;         // STACK: this frame's deferred list: count, then one slot per item handed to RESTART
    uint32_t *next_defer_count;  // STACK: count word of the other list (lists alternate between frames)
};
// A trace launch as it will be made.  STACK: the slot of its kernel (trace_slot), the dynamic LDS of a workgroup and the pixel
// slots a wave claims at a time; RESTART: the workgroups alone.
struct TraceLaunch {
    TraceChoice choice;
    uint32_t slot, blocks, lds_bytes, strip_items;
};

hipError_t launch_build_top_table(const uint32_t *nodes, uint32_t n_words, uint32_t *top_table,
                                  hipStream_t stream);
// plan_trace asks the runtime for the kernel's resident workgroups per CU the first time a context launches it, and launches nothing
hipError_t plan_trace(const TraceArgs &args, const LaunchInfo &li, const TraceChoice &choice, TraceLaunch &launch);
hipError_t launch_trace(const TraceArgs &args, const LaunchInfo &li, const TraceLaunch &launch, hipStream_t stream);
// after a STACK trace: deferred rays, per-strip costs (cost != nullptr) and the next schedule; re-arms the counters
constexpr uint32_t kMaxScheduledStrips = 1u << 20;  // (2^26 items / 64)
// cost class of a strip = (largest step count among its rays) >> kCostShift: 4 steps per class -- with 8 the cheapest two classes of the
// benchmark view hold 3 439 of 32 400 strips, fewer than the grid has waves, so every wave's last strip came from the 16..23-step
// class in screen order; the finer classes end the lists with the strips that really are the shortest
#ifndef SVO_COST_SHIFT
#define SVO_COST_SHIFT 2
#endif
constexpr uint32_t kCostShift = SVO_COST_SHIFT, kCostClasses = 128u >> SVO_COST_SHIFT;
constexpr uint32_t kOrderHistWords = 64 * kCostClasses;  // chunk histograms of the schedule builder, stored behind the class bytes
// (the list-share feedback's balance words, kBalance*: svo_sched.h, beside the share step)
// entries reserved per list of a schedule: a list holds its share of every cost class -- an eighth, or what the feedback gives it.
// The bound this needs: no list's share exceeds 2/8 (16384 of 65536).  Then its part of class c is at most
// (total_c * 16384 + 32768 >> 16) + 1 <= total_c / 4 + 1 strips after both of its bounds are rounded, n / 4 + kCostClasses over all
// classes.  The share step's constants kShareMin, kShareMax and kShareStepMin give it: the proof is beside balance_share_step in
// svo_sched.h; tests/test_sched_host.py holds the step to the bound and the list build to the cap.
inline uint32_t order_list_cap(uint32_t n_strips) { return (n_strips + 3u) / 4u + kCostClasses; }
// blocks per row for the schedule builder's column-major ranks (0: rank in strip order): frames of one rectangle of whole pixel blocks
inline uint32_t order_bpr(const WorkDesc &w, uint32_t n_strips) {
    if (w.mode == 2 || w.n_rects > 1u || w.bpr == 0u || n_strips % w.bpr != 0u || n_strips * 64u != w.n_items) return 0u;
    return w.bpr;
}
// the device buffers of one schedule slot (svo_ctx::Sched)
struct SchedBuffers {
    uint8_t *cost;      // the strips' cost classes; kOrderHistWords words of chunk histograms behind them
    uint8_t *cls_now;   // this frame's classes (filtered lists, motion floor); same layout
    uint32_t *order;    // 8 list lengths, then 8 lists of order_list_cap entries
    uint32_t *balance;  // kBalanceWords
};
hipError_t launch_post(const TraceArgs &args, const LaunchInfo &li, const PostPlan &plan, const SchedBuffers &buf, hipStream_t stream);
// svo_sched.hip: launch_post's list build (args.order_cap entries per list, shares from args.balance)
hipError_t launch_build_lists(const TraceArgs &args, uint32_t motion_floor, const SchedBuffers &buf, hipStream_t stream);

// svo_deal.hip: a resting view's static deal (svo_deal.h), one workgroup each on `stream`: seed the table from the stored lists (bal: the
// balance words the claiming kernel left the frame before);
// step it after a replayed frame (bal: the schedule's balance words); re-seed it if the rebuilt lists are not the ones it came from
struct Deal;
hipError_t launch_deal_seed(const Deal &d, const uint32_t *order, const uint32_t *bal, hipStream_t stream);
hipError_t launch_deal_step(const Deal &d, const uint32_t *bal, hipStream_t stream);
hipError_t launch_deal_compare(const Deal &d, const uint32_t *order, hipStream_t stream);

// explicit rays with a skip mask (args.skip): this frame's strip lists without the strips that hold no ray (classes from `prev`, or
// screen order)
hipError_t launch_schedule_skipping(const TraceArgs &args, const uint8_t *prev, uint8_t *cls, uint32_t *sched, uint32_t n_strips,
                                    uint32_t cap, hipStream_t stream);
// pixel frames seen from outside the cube: this frame's strip lists without the strips whose rays all miss it (their all-zero
// records are written here); args carries the work layout, the uniforms and the output buffers of the trace that follows
hipError_t launch_schedule_culling(const TraceArgs &args, const uint8_t *prev, uint8_t *cls, uint32_t *sched, uint32_t n_strips,
                                   uint32_t cap, hipStream_t stream);
// secondary rays of the hit pixels of args.hits; pixels without a hit get skip = 1 and a zero record in `out` instead of a ray
// (rays k_first .. n_secondary - 1; slot of ray k of record r: (k - k_first) * n_records + r)
hipError_t launch_secondary_gen(const TraceArgs &args, const float *aux_t, float *rays, uint8_t *skip, svo_hit *out, uint32_t k_first,
                                uint32_t n_secondary, uint32_t n_records, hipStream_t stream);
hipError_t launch_shade(const TraceArgs &args, const svo_hit *shadow_hits, uint32_t *rgba, hipStream_t stream);
hipError_t launch_diag_gather(const uint32_t *buf, uint32_t n_words, uint32_t stride_words, uint32_t n_loads, uint32_t *sink,
                              hipStream_t stream);
hipError_t launch_scan(uint32_t *nodes, uint32_t n_words, uint32_t node_length, uint32_t *sub, uint32_t *unsub,
                       uint32_t capacity, bool clear_counters, hipStream_t stream);
hipError_t launch_assemble_tiles(const void *gathered, bool packed, svo_hit *frame, uint32_t world, uint32_t n_pad, uint32_t width,
                                 uint32_t height, uint32_t tile_w, uint32_t tile_h, hipStream_t stream);
hipError_t launch_assemble_tiles_rgba(const uint32_t *gathered, uint32_t *frame, uint32_t world, uint32_t n_pad, uint32_t width,
                                      uint32_t height, uint32_t tile_w, uint32_t tile_h, hipStream_t stream);
hipError_t launch_pack_records(const svo_hit *records, uint32_t *wire, uint32_t n, hipStream_t stream);
hipError_t launch_scatter(uint32_t *nodes, uint32_t n_words, const uint32_t *indices, const uint32_t *words, uint32_t n,
                          hipStream_t stream);

}  // namespace svo

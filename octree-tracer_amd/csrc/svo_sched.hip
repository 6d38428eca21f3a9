// svo_sched.hip -- the strip schedule's list builders: cost classes -> 8 per-XCD strip lists, longest strips
// first, for the trace kernel (svo_kernels.hip) to claim from.  Which of them run for a frame is decided by svo_sched.h; the post pass
// that measures the costs (post_kernel) and the list-share step (balance_step) stay beside the trace kernel.
#include <hip/hip_runtime.h>

#include "svo_device.h"
#include "svo_trace_fn.h"

namespace svo {

// Schedule for the next frames.  Strips fall into 16 cost classes (steps / 8).  Classes are walked from the
// most expensive down; inside a class the strips stay in screen order and are cut into 8 contiguous
// segments, one per claim counter (= per XCD, see the kernel).  So every XCD starts its long rays first,
// gets an equal share of every class, and still walks screen-contiguous runs (node-cache locality).
// Output: sched[0..7] = entries per list, then 8 lists of `cap` strip numbers each.
// Two small launches over kOrderBlocks workgroups, each owning a contiguous chunk of strips: class histogram
// per chunk, then a stable counting sort (ballot + mbcnt ranks inside a wave, prefix over waves and chunks).
constexpr uint32_t kOrderBlocks = 64, kOrderThreads = 256, kOrderBins = kCostClasses, kOrderLists = 8;

__device__ __forceinline__ uint32_t order_chunk(uint32_t n_strips) {
    return (((n_strips + kOrderBlocks - 1) / kOrderBlocks) + 63u) & ~63u;  // whole 64-strip groups per workgroup
}

// Round 5: the strips of a class are ranked COLUMN by column when the frame is one rectangle of pixel blocks (bpr = blocks per row, else
// 0: strip order): a list's segment of a class is then a vertical slab of the screen, and the slabs of the different classes of one list
// overlap -- the lists (one per XCD, each with an L2 of its own) share fewer nodes: 225 k instead of 272 k cache lines fetched per
// frame by the eight L2s together on the benchmark frame (180 k distinct; row-major ranks cut every class into horizontal bands that
// lie elsewhere for every class), profiles/r05_footprint_by_partition.txt.
__device__ __forceinline__ uint32_t order_strip_at(uint32_t p, uint32_t n_strips, uint32_t bpr) {
    if (bpr == 0u) return p;
    const uint32_t rows = n_strips / bpr;  // (the caller passes bpr only when n_strips is rows * bpr)
    const uint32_t col = p / rows;
    return (p - col * rows) * bpr + col;
}

__global__ __launch_bounds__(kOrderThreads) void strip_hist_kernel(const uint8_t *cls, uint32_t n_strips, uint32_t *hist, uint32_t bpr) {
    __shared__ uint32_t tally[kOrderBins];
    if (threadIdx.x < kOrderBins) tally[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t chunk = order_chunk(n_strips);
    const uint32_t lo = min(blockIdx.x * chunk, n_strips), hi = min(lo + chunk, n_strips);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = lo + (threadIdx.x & ~63u); base < hi; base += kOrderThreads) {
        const uint32_t s = base + lane;
        const uint32_t c = s < hi ? cls[order_strip_at(s, n_strips, bpr)] : 0xFFu;
        uint64_t todo = __ballot(c != 0xFFu);
        while (todo) {  // one LDS atomic per (wave, class present) instead of one per strip
            const uint32_t b = __builtin_amdgcn_readlane(c, __ffsll((unsigned long long)todo) - 1);
            const uint64_t m = __ballot(c == b);
            if (lane == 0) atomicAdd(&tally[b], (uint32_t)__popcll(m));
            todo &= ~m;
        }
    }
    __syncthreads();
    if (threadIdx.x < kOrderBins) hist[blockIdx.x * kOrderBins + threadIdx.x] = tally[threadIdx.x];
}

__global__ __launch_bounds__(kOrderThreads) void strip_order_kernel(const uint8_t *cls, const uint32_t *hist, uint32_t *sched,
                                                                    uint32_t n_strips, uint32_t cap, uint32_t bpr, const uint32_t *shares) {
    constexpr uint32_t kWaves = kOrderThreads / 64;
    __shared__ uint32_t class_n[kOrderBins], before[kOrderBins];
    // bound[c][k]: rank (inside class c) of the first strip that goes to list k -- equal eighths, or the shares of the lists
    // (`shares`: nine cumulative 16-bit fractions 0 .. 65536, from the times the lists took in an earlier frame: see launch_post)
    __shared__ uint32_t bound[kOrderBins][kOrderLists + 1];
    __shared__ uint32_t list_base[kOrderBins][kOrderLists];
    __shared__ uint32_t wave_tot[kOrderBins][kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid < kOrderBins) {  // class totals and the count in the chunks before this one
        uint32_t total = 0, prior = 0;
        for (uint32_t b = 0; b < kOrderBlocks; b++) {
            const uint32_t c = hist[b * kOrderBins + tid];
            prior += b < blockIdx.x ? c : 0u;
            total += c;
        }
        class_n[tid] = total;
        before[tid] = prior;
        for (uint32_t k = 0; k <= kOrderLists; k++) {
            const uint32_t frac = shares ? shares[k] : (k << 16) / kOrderLists;
            bound[tid][k] = k == kOrderLists ? total : (uint32_t)(((uint64_t)total * frac + 32768u) >> 16);
        }
    }
    __syncthreads();
    if (tid < kOrderLists) {
        uint32_t acc = 0;
        for (int b = kOrderBins - 1; b >= 0; b--) {  // expensive classes first
            list_base[b][tid] = acc;
            acc += bound[b][tid + 1] - bound[b][tid];
        }
        if (blockIdx.x == 0) sched[tid] = min(acc, cap);
    }
    // each wave owns a contiguous run of 64-strip groups of the chunk; lanes 0..31 keep the class tallies
    const uint32_t chunk = order_chunk(n_strips);
    const uint32_t clo = min(blockIdx.x * chunk, n_strips), chi = min(clo + chunk, n_strips);
    const uint32_t per_wave = (((chunk / 64u) + kWaves - 1) / kWaves) * 64u;
    const uint32_t lo = min(clo + wv * per_wave, chi), hi = min(lo + per_wave, chi);
    uint32_t tally = 0;
    for (uint32_t base = lo; base < hi; base += 64u) {
        const uint32_t s = base + lane;
        const uint32_t c = s < hi ? cls[order_strip_at(s, n_strips, bpr)] : 0xFFu;
        uint64_t todo = __ballot(c != 0xFFu);
        while (todo) {
            const uint32_t b = __builtin_amdgcn_readlane(c, __ffsll((unsigned long long)todo) - 1);
            const uint64_t m = __ballot(c == b);
            if (lane == b) tally += (uint32_t)__popcll(m);
            todo &= ~m;
        }
    }
    if (lane < kOrderBins) wave_tot[lane][wv] = tally;
    __syncthreads();
    uint32_t run = 0;  // rank (inside its class) of the wave's next strip of class `lane`
    if (lane < kOrderBins) {
        run = before[lane];
        for (uint32_t w = 0; w < wv; w++) run += wave_tot[lane][w];
    }
    for (uint32_t base = lo; base < hi; base += 64u) {
        const uint32_t s = order_strip_at(base + lane, n_strips, bpr);  // (positions past the chunk's end are not looked at)
        const uint32_t c = base + lane < hi ? cls[s] : 0xFFu;
        uint64_t todo = __ballot(c != 0xFFu);
        uint32_t rank = 0;
        while (todo) {
            const uint32_t b = __builtin_amdgcn_readlane(c, __ffsll((unsigned long long)todo) - 1);
            const uint64_t m = __ballot(c == b);
            const uint32_t first = __builtin_amdgcn_readlane(run, b);
            if (c == b)
                rank = first + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (lane == b) run += (uint32_t)__popcll(m);
            todo &= ~m;
        }
        if (c != 0xFFu) {
            uint32_t list = 0;
#pragma unroll
            for (uint32_t k = 1; k < kOrderLists; k++) list += rank >= bound[c][k] ? 1u : 0u;
            const uint32_t at = list_base[c][list] + (rank - bound[c][list]);
            if (at < cap) sched[kOrderLists + list * cap + at] = s;  // (cap: order_list_cap, which bounds a list's share)
        }
    }
}

// Explicit rays with a skip mask (secondary rays: most slots of a frame can be empty): cost classes for THIS frame's
// schedule -- 0xFF, which strip_order_kernel leaves out of the lists, for strips without a single ray, else the class the
// strip had when costs were last measured (0 when there is no measurement: screen order) -- and the lists built from
// them.  Strips that are not in a list are never claimed, so empty slots cost the trace nothing.
__global__ __launch_bounds__(256) void strip_classes_kernel(const uint8_t *skip, uint32_t n_items, const uint8_t *prev, uint8_t *cls,
                                                            uint32_t n_strips) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_strips) return;
    bool empty = true;
    if ((uint64_t)s * 64u + 64u <= n_items) {
        const uint4 *p = reinterpret_cast<const uint4 *>(skip + (uint64_t)s * 64u);  // the mask is 256-byte aligned (hipMalloc)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = p[i];  // the producer writes 0 or 1
            empty = empty && v.x == 0x01010101u && v.y == 0x01010101u && v.z == 0x01010101u && v.w == 0x01010101u;
        }
    } else {
        for (uint32_t q = s * 64u; q < n_items; q++) empty = empty && skip[q] != 0u;
    }
    cls[s] = empty ? (uint8_t)0xFFu : (prev ? prev[s] : (uint8_t)0u);
}

// Strips whose rays all miss the cube (sky): decided per 64-pixel block from the four corner rays, before the trace, so
// that such strips are never claimed, generated or refilled from -- on frames that are mostly sky that is most of the
// per-strip work.  The rays of a block are pos + s * (point(pixel) - pos), s > 0, where point() is the
// projective image of the pixel under camera_inverse: the block's points lie in the planar convex quadrilateral Q of its
// four corner pixels (same sign of w at the corners), so every ray lies in the cone over Q with apex pos.  If one side
// plane of that cone (through pos and an edge of Q, normal n pointing into the cone) has the whole cube strictly on its
// outer side -- max over the cube's corners of n.(v - pos) = |n.x| + |n.y| + |n.z| - n.pos < -margin -- no ray of the block
// meets the cube and ray_box_dist returns 0 for each of them (shader.wgsl:66-80: v7 > v8).  The margin (1e-3 of the
// plane function's scale, ~1e-3 rad) is four orders of magnitude above the rounding of either computation: blocks
// anywhere near the cube's silhouette are NOT culled and take the ordinary path.  A culled strip's 64 records are what
// the trace writes for rays that never enter the cube: all zeros.
// (One LANE per strip for the test -- the pixel bounds of a block follow from its position, no reduction over its pixels is
// needed -- and one wave-wide pass per culled strip for its 64 zero records: with one wave per strip, every lane repeating the
// four corner rays, the pass took 32 us per 1080p frame, a third of the trace it saves on.)
__global__ __launch_bounds__(256) void strip_cull_kernel(TraceArgs a, const uint8_t *prev, uint8_t *cls, uint32_t n_strips) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, n_waves = gridDim.x * 4u;
    const WorkDesc &w = a.work;
    float p4[4];
    mat_vec(a.u.camera_inverse, 0.0f, 0.0f, 0.0f, 1.0f, p4);
    const float o0 = p4[0] / p4[3], o1 = p4[1] / p4[3], o2 = p4[2] / p4[3];
    for (uint32_t base = wave * 64u; base < n_strips; base += n_waves * 64u) {
        const uint32_t s = base + lane;
        bool culled = false;
        if (s < n_strips) {
            // the block's first pixel and how many of its columns and rows lie inside the rectangle
            const ItemFast it0 = decode_item_fast(w, s * 64u);
            uint32_t x_lo = 0u, x_hi = 0u, y_lo = 0u, y_hi = 0u;
            bool any = it0.valid;
            if (any) {
                const uint32_t blk = s, rect = w.n_rects > 1u ? fast_div(blk, w.bprect, w.magic_bprect) : 0u, b = blk - rect * w.bprect;
                const uint32_t by = fast_div(b, w.bpr, w.magic_bpr), bx = b - by * w.bpr;
                const uint32_t x = bx << w.bw_log2, y = by << (6u - w.bw_log2);
                x_lo = it0.px; y_lo = it0.py;
                x_hi = it0.px + min((1u << w.bw_log2) - 1u, w.w - 1u - x);
                y_hi = it0.py + min((1u << (6u - w.bw_log2)) - 1u, w.h - 1u - y);
            }
            if (any) {
                // corner k of the quadrilateral, in order around it: (lo,lo) (hi,lo) (hi,hi) (lo,hi)
                float q[4][3];
                bool ok = true;
                float wsign = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t px = (k == 1 || k == 2) ? x_hi : x_lo, py = (k >= 2) ? y_hi : y_lo;
                    const float cx = ((float)px + 0.5f) / a.u.dimensions[0] * 2.0f - 1.0f;
                    const float cy = -(((float)py + 0.5f) / a.u.dimensions[1] * 2.0f - 1.0f);
                    float d4[4];
                    mat_vec(a.u.camera_inverse, cx, cy, 1.0f, 1.0f, d4);
                    q[k][0] = d4[0] / d4[3] - o0; q[k][1] = d4[1] / d4[3] - o1; q[k][2] = d4[2] / d4[3] - o2;
                    ok = ok && fabsf(d4[3]) > 1.0e-20f && (k == 0 || (d4[3] > 0.0f) == (wsign > 0.0f));
                    wsign = d4[3];
                }
                ok = ok && fabsf(p4[3]) > 1.0e-20f;
                if (ok) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float *u = q[k], *v = q[(k + 1) & 3], *ww = q[(k + 2) & 3];
                        float n0 = u[1] * v[2] - u[2] * v[1], n1 = u[2] * v[0] - u[0] * v[2], n2 = u[0] * v[1] - u[1] * v[0];
                        const float inside = n0 * ww[0] + n1 * ww[1] + n2 * ww[2];  // the opposite corner is inside the cone
                        if (inside < 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
                        const float reach = fabsf(n0) + fabsf(n1) + fabsf(n2);
                        const float at_pos = n0 * o0 + n1 * o1 + n2 * o2;
                        const float scale = reach + fabsf(n0 * o0) + fabsf(n1 * o1) + fabsf(n2 * o2);
                        // a degenerate quadrilateral (inside == 0: a one-pixel-wide strip) or NaNs leave every comparison false
                        if (fabsf(inside) > 0.0f && reach - at_pos < -1.0e-3f * scale) culled = true;
                    }
                }
            }
            cls[s] = culled ? (uint8_t)0xFFu : (prev ? prev[s] : (uint8_t)0u);
        }
        // the zero records of the culled strips, one strip at a time, one record per lane
        uint64_t todo = __ballot(culled);
        while (todo) {
            const uint32_t t = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
            todo &= todo - 1ull;
            const ItemFast it = decode_item_wave(w, (base + t) * 64u, lane);
            if (it.valid) {
                reinterpret_cast<uint4 *>(a.hits)[it.out] = make_uint4(0u, 0u, 0u, 0u);
                if (a.aux_t) a.aux_t[it.out] = 0.0f;
                if (a.shadow_hits) reinterpret_cast<uint4 *>(a.shadow_hits)[it.out] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
    }
}

// the two kernels of the schedule builder for the class bytes `cls` (the chunk histograms live behind them)
static void launch_order_pair(const WorkDesc &w, const uint8_t *cls, uint32_t *sched, uint32_t n_strips, uint32_t cap, hipStream_t stream,
                              const uint32_t *shares = nullptr) {
    uint32_t *hist = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(cls) + ((n_strips + 15u) & ~15u));
    const uint32_t bpr = order_bpr(w, n_strips);
    hipLaunchKernelGGL(strip_hist_kernel, dim3(kOrderBlocks), dim3(kOrderThreads), 0, stream, cls, n_strips, hist, bpr);
    hipLaunchKernelGGL(strip_order_kernel, dim3(kOrderBlocks), dim3(kOrderThreads), 0, stream, cls, (const uint32_t *)hist, sched, n_strips, cap, bpr, shares);
}

// This frame's strip lists without the culled strips (classes from `prev`, or screen order); see launch_schedule_skipping.
hipError_t launch_schedule_culling(const TraceArgs &args, const uint8_t *prev, uint8_t *cls, uint32_t *sched, uint32_t n_strips,
                                   uint32_t cap, hipStream_t stream) {
    (void)hipGetLastError();
    uint32_t blocks = (n_strips + 255u) / 256u;  // a lane per strip
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(strip_cull_kernel, dim3(blocks), dim3(256), 0, stream, args, prev, cls, n_strips);
    launch_order_pair(args.work, cls, sched, n_strips, cap, stream);
    return hipGetLastError();
}

hipError_t launch_schedule_skipping(const TraceArgs &args, const uint8_t *prev, uint8_t *cls, uint32_t *sched, uint32_t n_strips,
                                    uint32_t cap, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(strip_classes_kernel, dim3((n_strips + 255u) / 256u), dim3(256), 0, stream, args.skip, args.work.n_items, prev, cls,
                       n_strips);
    launch_order_pair(args.work, cls, sched, n_strips, cap, stream);  // (explicit rays: strip order)
    return hipGetLastError();
}

// Cost classes for a camera that MOVES.  The strips that decide a frame hold a ray that runs into the step limit; those rays
// are isolated pixels, and which pixels they are changes with a sub-pixel change of the view: the class a strip
// had one frame ago says little about whether it holds one now.  Where they can be does carry over -- they come in regions
// (grazing views of the terrain), other regions (sky, near surfaces seen head-on) have none.  A strip with at least
// `min_count` such strips among its (2 radius + 1)^2 neighbours is therefore given at least class `floor_class`: "cheap, but
// one in ten of its kind turns out to take the whole frame" sorts before "cheap" without getting ahead of the strips that
// were measured long.
__global__ __launch_bounds__(256) void strip_danger_kernel(const uint8_t *in, uint8_t *out, uint32_t n_strips, uint32_t bpr, int radius,
                                                           uint32_t min_count, uint32_t floor_class) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_strips) return;
    const int by = (int)(s / bpr), bx = (int)(s - (uint32_t)by * bpr), rows = (int)((n_strips + bpr - 1u) / bpr);
    uint32_t c = in[s], near = 0u;
    if (c < floor_class) {
        for (int dy = -radius; dy <= radius; dy++)
            for (int dx = -radius; dx <= radius; dx++) {
                const int y = by + dy, x = bx + dx;
                if (y < 0 || y >= rows || x < 0 || x >= (int)bpr) continue;
                const uint32_t t = (uint32_t)y * bpr + (uint32_t)x;
                if (t < n_strips && in[t] >= (64u >> kCostShift)) near++;  // a ray of 64 steps or more
            }
        if (near >= min_count) c = floor_class;
    }
    out[s] = (uint8_t)c;
}


// The lists for the next frames, from the costs the post pass measured (motion_floor != 0: floored into `buf.cls_now` first).
hipError_t launch_build_lists(const TraceArgs &args, uint32_t motion_floor, const SchedBuffers &buf, hipStream_t stream) {
    const uint32_t n_strips = (args.work.n_items + 63u) / 64u;
    const uint8_t *cls = buf.cost;
    if (motion_floor) {  // (pixel frames of one rectangle: the policy sets the floor only then)
        hipLaunchKernelGGL(strip_danger_kernel, dim3((n_strips + 255u) / 256u), dim3(256), 0, stream, (const uint8_t *)buf.cost, buf.cls_now,
                           n_strips, args.work.bpr, (int)((motion_floor >> 8) & 15u), (motion_floor >> 12) & 255u,
                           ((motion_floor & 15u) << 3) >> kCostShift);  // (the option counts the floor in units of 8 steps)
        cls = buf.cls_now;
    }
    // (the chunk histograms live behind the class bytes: SchedBuffers allocates kOrderHistWords extra words)
    launch_order_pair(args.work, cls, buf.order, n_strips, args.order_cap, stream, args.balance);
    return hipGetLastError();
}

}  // namespace svo

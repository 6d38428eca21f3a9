// svo_region.hip -- the tree in the node buffer edited by shapes: boxes and balls filled, carved and
// painted, top-down, so that only the words along the shapes' surfaces are looked at.  include/svo_hip.h has the rule for
// one word; this file applies it level by level.  Scans instead of atomics, integers instead of floats: the words do not
// depend on the run.
//
// The walk is svo_frontier.h's: frontier, scans, check, status and commit; this file has the plan.
//
//   plan      per level, reading only, one lane per frontier word: the shapes, staged in LDS once per workgroup, are
//             classified against the word's cube from the last to the first, until one that covers the cube in SET mode ends
//             the loop; a leaf that shapes behind it touch goes through those forwards.  The lane flags its word opened or
//             split and puts what it would write into the write list
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_ctx.h"
#include "svo_frontier.h"  // (the walk: Entry, PlanOut, emit_head, Walk; kNone, leaf_word, mode_applies)

static_assert(sizeof(svo_region_shape) == 32, "a shape is two uint4 in LDS");

namespace {

enum Class : uint32_t { kOut, kPart, kFull };

// One axis of a ball against the cells [c0, c0 + 2^s): the distances of the farthest and the nearest cell centre from
// the ball's centre C, in half cells, squared and added up.
__host__ __device__ inline void ball_axis(uint32_t c0, uint32_t s, uint32_t C, int64_t &far, int64_t &near) {
    const int64_t lo = 2 * int64_t(c0) + 1 - int64_t(C), hi = 2 * (int64_t(c0) + (int64_t(1) << s)) - 1 - int64_t(C);  // lo <= hi
    const int64_t f = -lo > hi ? -lo : hi;
    const int64_t n = lo > 0 ? lo : hi < 0 ? -hi : (C & 1u) ? 0 : 1;
    far += f * f;
    near += n * n;
}

__host__ __device__ inline bool box_axis_out(uint32_t c0, uint32_t s, uint32_t lo, uint32_t hi) { return c0 + (1u << s) <= lo || c0 >= hi; }
__host__ __device__ inline bool box_axis_full(uint32_t c0, uint32_t s, uint32_t lo, uint32_t hi) { return lo <= c0 && c0 + (1u << s) <= hi; }

// The shape {kind | mode << 16, colour, a[0], a[1]}, {a[2], b[0], b[1], b[2]} against the cube of 2^s cells at (x, y, z).
__host__ __device__ inline uint32_t shape_class(const uint4 &p, const uint4 &q, uint32_t x, uint32_t y, uint32_t z, uint32_t s) {
    if ((p.x & 0xFFFFu) == SVO_REGION_BOX) {
        if (box_axis_out(x, s, p.z, q.y) || box_axis_out(y, s, p.w, q.z) || box_axis_out(z, s, q.x, q.w)) return kOut;
        return box_axis_full(x, s, p.z, q.y) && box_axis_full(y, s, p.w, q.z) && box_axis_full(z, s, q.x, q.w) ? kFull : kPart;
    }
    int64_t far = 0, near = 0;
    ball_axis(x, s, p.z, far, near);
    ball_axis(y, s, p.w, far, near);
    ball_axis(z, s, q.x, far, near);
    const int64_t r2 = int64_t(q.y) * int64_t(q.y);
    return near > r2 ? kOut : far <= r2 ? kFull : kPart;
}

// The rule for the frontier words of `level` (dynamic LDS: 2 * n_shapes uint4); a word that would be opened at level ==
// depth is refused.
__global__ __launch_bounds__(kThreads) void region_plan_kernel(const uint32_t *__restrict__ words, const uint4 *__restrict__ shapes,
                                                               uint32_t n_shapes, uint32_t depth, uint32_t level, Frontier f, PlanOut o) {
    extern __shared__ __attribute__((aligned(16))) uint4 sh[];  // (behind block_min's 1 KB of static LDS: 16-byte aligned)
    for (uint32_t t = threadIdx.x; t < 2u * n_shapes; t += kThreads) sh[t] = shapes[t];
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, s = depth - level;
    uint32_t refused = kNone;
    if (i < f.n) {
        const Entry e = frontier_entry(words, f, i);
        const uint32_t x = e.x << s, y = e.y << s, z = e.z << s;
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        // from the last shape to the first: j covers the cube in SET mode; `last` is the last shape behind j that touches it
        uint32_t j = kNone, last = kNone;
        for (uint32_t k = n_shapes; k-- > 0;) {
            const uint4 p = sh[2 * k];
            const uint32_t cls = shape_class(p, sh[2 * k + 1], x, y, z, s);
            if (cls == kOut) continue;
            if (cls == kFull && (p.x >> 16) == SVO_REGION_SET) {
                j = k;
                break;
            }
            if (last == kNone) last = k;
        }
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (!leaf) {
            if (last != kNone) {
                if (level == depth) refused = i;
                else cd = kOpen;
            } else if (j != kNone) {  // collapse
                at = e.at;
                out = leaf_word(sh[2 * j].y & 0xFFFFFFu);
            }
        } else if (j != kNone || last != kNone) {
            const uint32_t v0 = (e.word >> 4) - SVO_VOXEL_OFFSET;
            uint32_t v = j != kNone ? sh[2 * j].y & 0xFFFFFFu : v0;
            bool split = false;
            if (last != kNone)
                for (uint32_t k = j + 1u; k <= last; k++) {  // (j == kNone: from 0)
                    const uint4 p = sh[2 * k];
                    const uint32_t colour = p.y & 0xFFFFFFu;
                    if (!mode_applies(p.x >> 16, v) || colour == v) continue;
                    const uint32_t cls = shape_class(p, sh[2 * k + 1], x, y, z, s);
                    if (cls == kFull) v = colour;
                    else if (cls == kPart) {
                        split = true;
                        break;
                    }
                }
            if (split && level < depth) {  // (at level == depth nothing is PART)
                cd = kOpen | kSplit;
                at = e.at;
                fill = e.word & ~15u;
            } else if (!split && v != v0) {
                at = e.at;
                out = leaf_word(v);
            }
        }
        plan_store(o, i, cd, at, out, fill);
    }
    plan_refused(o, refused);
}

// Behind the two scans: the records of the next frontier's groups, in the order of their parents.
__global__ __launch_bounds__(kThreads) void region_emit_kernel(const uint32_t *__restrict__ words, Frontier f, EmitArgs a) {
    Opened o;
    if (emit_head(words, f, a, o)) emit_record(a, o);
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// What the shape edit keeps per context beside the walk's workspace (svo_ctx::region): the shapes and the times.
struct svo_region_state {
    svo_pinned<uint4> shapes_host;
    svo_dev<uint4> shapes;
    svo_pass_timer<kEvs, SVO_REGION_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        HIP_TRY(ctx, shapes_host.alloc(2 * SVO_REGION_MAX_SHAPES));
        HIP_TRY(ctx, shapes.alloc(2 * SVO_REGION_MAX_SHAPES));
        return SVO_OK;
    }
};

namespace {

int check_shapes(svo_ctx *ctx, const svo_region_shape *shapes, size_t n, uint32_t depth) {
    const uint64_t side = 1ull << depth;
    for (size_t k = 0; k < n; k++) {
        const svo_region_shape &s = shapes[k];
        const std::string who = "shape " + std::to_string(k);
        if (s.kind != SVO_REGION_BOX && s.kind != SVO_REGION_BALL) return svo_fail(ctx, SVO_ERR_ARG, who + ": unknown kind " + std::to_string(s.kind));
        if (s.mode < 1 || s.mode > 3) return svo_fail(ctx, SVO_ERR_ARG, who + ": mode must be 1..3 (got " + std::to_string(s.mode) + ")");
        for (int a = 0; a < 3; a++) {
            if (s.kind == SVO_REGION_BOX && (s.a[a] >= s.b[a] || s.b[a] > side))
                return svo_fail(ctx, SVO_ERR_ARG, who + ": a box needs lo < hi <= 2^depth on every axis (axis " + std::to_string(a) + ": lo " +
                                                      std::to_string(s.a[a]) + ", hi " + std::to_string(s.b[a]) + ", depth " + std::to_string(depth) + ")");
            if (s.kind == SVO_REGION_BALL && s.a[a] > 2 * side)
                return svo_fail(ctx, SVO_ERR_ARG, who + ": a ball's centre lies in [0, 2^(depth+1)] half cells (axis " + std::to_string(a) + ": " +
                                                      std::to_string(s.a[a]) + ", depth " + std::to_string(depth) + ")");
        }
        if (s.kind == SVO_REGION_BALL && s.b[0] > (1u << 23))
            return svo_fail(ctx, SVO_ERR_ARG, who + ": a ball's radius is at most 2^23 half cells (got " + std::to_string(s.b[0]) + ")");
    }
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_nodes_edit_region(svo_ctx *ctx, const svo_region_shape *shapes, size_t n_shapes, const svo_region_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (n_shapes && !shapes) return svo_fail(ctx, SVO_ERR_ARG, "null shapes");
    if (n_shapes > SVO_REGION_MAX_SHAPES)
        return svo_fail(ctx, SVO_ERR_ARG, std::to_string(n_shapes) + " shapes, more than SVO_REGION_MAX_SHAPES = " + std::to_string(SVO_REGION_MAX_SHAPES));
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc || (rc = check_shapes(ctx, shapes, n_shapes, p->depth)) || (rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a shape edit cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->region))) return rc;
    svo_region_state *s = ctx->region.get();
    if (!n_shapes) {  // nothing to edit
        s->timer.none();
        *n_words_out = p->n_words;
        return SVO_OK;
    }
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t depth = p->depth, n_sh = (uint32_t)n_shapes;
    struct : FrontierPass {
        svo_region_state *s;
        uint32_t n_sh, depth;
        void plan(svo_ctx *ctx, const Level &l) {
            region_plan_kernel<<<l.blocks, kThreads, n_sh * sizeof(svo_region_shape), ctx->stream>>>(ctx->nodes, s->shapes, n_sh, depth, l.level, l.at, l.out);
        }
        void emit(svo_ctx *ctx, const Level &l) { region_emit_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, l.at, l.emit); }
    } pass;
    pass.s = s, pass.n_sh = n_sh, pass.depth = depth;
    Walk walk;
    if ((rc = walk.begin(ctx, p->n_words, depth, "edited", s->timer.ev[kEvStart]))) return rc;
    memcpy(s->shapes_host.get(), shapes, n_shapes * sizeof(svo_region_shape));
    HIP_TRY(ctx, hipMemcpyAsync(s->shapes, s->shapes_host, n_shapes * sizeof(svo_region_shape), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = walk.run(ctx, pass, s->timer.ev[kEvPlan], s->timer.ev[kEvStatus]))) return rc;
    if (walk.refused) {
        // the last shape that touches the refused cell, found again on the host
        const Cell c = walk.cell;
        const uint4 *sh = s->shapes_host;
        size_t k = n_shapes;
        while (k-- > 0 && shape_class(sh[2 * k], sh[2 * k + 1], c.x, c.y, c.z, 0) == kOut) {}
        return svo_fail(ctx, SVO_ERR_STATE, "shape " + std::to_string(k) + " meets cell (" + std::to_string(c.x) + ", " + std::to_string(c.y) + ", " +
                                                std::to_string(c.z) + "), which is an interior node at depth " + std::to_string(depth) +
                                                ": the tree is finer there than the edit, and the shape does not replace the subtree");
    }
    if ((rc = walk.commit(ctx, p->max_words, s->timer.ev[kEvFill], s->timer.ev[kEvEnd], n_words_out))) return rc;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_region_timing(svo_ctx *ctx, float ms_out[SVO_REGION_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->region) return svo_fail(ctx, SVO_ERR_STATE, "no tree edited by shapes on this context yet");
    return ctx->region->timer.read(ctx, ms_out);
}

}  // extern "C"

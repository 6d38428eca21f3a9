// svo_transform.hip -- a tree placed into the scene under any fixed-point affine map from scene cells to source cells, sampled at
// cell centres, nearest cell: the placement (svo_place.hip) with the signed permutation replaced by
// a matrix, so free turns, scale and shear, and a source whose cells are not the scene's.  include/svo_hip.h has the rule for one
// word; this file applies it level by level with the walk of svo_frontier.h and the combine's plan.  Where the
// placement inherits a word's items from its parent's, this pass finds them by geometry:
//
//   box       all source cells that the cells of a scene word can sample lie in a box, exact interval arithmetic over the
//             cube's cell centres: nine 32 x 32 -> 64 bit multiply-adds per word.  The matrix, twice the translation and the
//             level's radius are kernel arguments
//   items     the cells of the source's level-k grid that the box meets, k the deepest level whose cells are no smaller than
//             the box: at most two per axis.  One word each: OUT, a constant or a source interior word, found by a walk down
//             the source; folded into the placement's five counters as they are found, never kept in an array
//   hint      per frontier group, two u32: the deepest source node whose cell holds the parent's whole box, as a source word
//             without its counter, and its level.  A child's box lies in its parent's, so a child's walk starts there and
//             not at the root; the node's cell needs no coordinates, it is the cell of its level that holds the child's box.
//             A box that leaves the source's cube has the root, level 0
//   plan      per level, reading only, one lane per frontier word: from the hint down the path that all items share (the
//             levels on which the box's two corners lie in one cell), then each item from there; the items taken together
//             are nothing, one constant or a subtree, and from there on the lane is the combine's
//   pointers  every source pointer is checked before it is followed, by the lane that follows it, so a malformed source is
//             never read out of bounds; an interior item's pointer of a word that is opened or split is checked by the plan
//             as the placement's emit checks it, before the next level starts from it
//   emit      the next frontier's records with the hint of the opened word's own box
//
// No overflow: |matrix| <= 2^20, a doubled cell centre < 2^22 and |2 translate| <= 2^41 give |mid| < 3 * 2^42 + 2^41; zc <= 2^20
// from level 1 on gives rad <= (2^20 - 1) * 3 * 2^20 < 3 * 2^40; so |mid +- rad| < 4.25 * 2^42 < 2^45 and every source cell
// index is below 2^28 in magnitude.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_combine_rules.h"  // (combine_value, whole_subtree, whole_constant, leaf_stays; Src, kSceneFiner, kSourceFiner, kOpNames, SourcePass)
#include "svo_ctx.h"
#include "svo_frontier.h"  // (the walk: Entry, PlanOut, emit_head, Walk; kNone, leaf_word)

namespace {

constexpr int32_t kMaxEntry = 1 << 20;
constexpr int64_t kMaxTranslate = int64_t(1) << 40;
constexpr uint32_t kFraction = 17;  // P is 2^17 times the source point: Q16, and the doubled cell centre

// The call's constants and the level's, by value to the kernels: uniform, so in SGPRs.  t2: twice the translation; rad: the
// level's radius per source axis, (zc - 1) * sum_j |matrix[i][j]|; zc: the cells a side of a word of the level.
struct Facing {
    uint32_t op, depth, src_depth, src_words;
    int32_t m[9];
    uint32_t zc;
    int64_t t2[3], rad[3];
};

// the source cells that the cells of the level's word (x, y, z) can sample: lo..hi per source axis
struct Box {
    int32_t lo[3], hi[3];
};
__device__ inline Box word_box(const Facing &t, uint32_t x, uint32_t y, uint32_t z) {
    // the doubled centre of the word's cube in scene cells, below 2^22; every product below 2^42 (v_mad_i64_i32)
    const int64_t cx = int64_t((2u * x + 1u) * t.zc), cy = int64_t((2u * y + 1u) * t.zc), cz = int64_t((2u * z + 1u) * t.zc);
    Box b;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int64_t mid = int64_t(t.m[3 * i]) * cx + int64_t(t.m[3 * i + 1]) * cy + int64_t(t.m[3 * i + 2]) * cz + t.t2[i];
        b.lo[i] = int32_t((mid - t.rad[i]) >> kFraction);  // (arithmetic: floor; |.| < 2^28)
        b.hi[i] = int32_t((mid + t.rad[i]) >> kFraction);
    }
    return b;
}

// the bits of v: 0 for 0
__device__ inline uint32_t bits_of(uint32_t v) { return 32u - uint32_t(__clz(int(v))); }

// One step down the source: the interior word w becomes its child `child`, without the counter.  The pointer is checked as
// the discovery checks a scene's before anything behind it is read; false, with the status word set, when it is malformed.
__device__ inline bool src_step(const uint32_t *__restrict__ src, uint32_t src_words, uint32_t &w, uint32_t child, uint32_t *status) {
    const uint32_t pointer = w >> 4;
    if (pointer & 7u) {
        status[kStSrcAlign] = 1u;  // (every writer stores the same value)
        return false;
    }
    if (pointer + 8u > src_words) {  // (pointer < 2^28: no wrap)
        status[kStSrcRange] = 1u;
        return false;
    }
    w = src[pointer + child] & ~15u;
    return true;
}
__device__ inline bool src_interior(uint32_t w) { return (w >> 4) < SVO_VOXEL_OFFSET; }
// the child index, on the level whose cells have 2^sh cells of the finer grid a side, of the cell (x, y, z) of that grid
__device__ inline uint32_t child_of(int32_t x, int32_t y, int32_t z, uint32_t sh) {
    return (uint32_t(x) >> sh & 1u) << 2 | (uint32_t(y) >> sh & 1u) << 1 | (uint32_t(z) >> sh & 1u);
}

// From the group's hint (w at level m) down the path that the whole box shares: afterwards w at level m is the deepest source
// node whose cell holds the box, the root at level 0 for a box that leaves the source's cube.  The box lies in the hint's cell.
__device__ inline void shared_walk(const uint32_t *__restrict__ src, const Facing &t, const Box &b, uint32_t &w, uint32_t &m, uint32_t *status) {
    const int32_t side = int32_t(1u << t.src_depth);
    const bool inside = (b.lo[0] | b.lo[1] | b.lo[2]) >= 0 && b.hi[0] < side && b.hi[1] < side && b.hi[2] < side;
    if (!inside) return;  // (then the hint is the root: a node below it has its cell, and the box with it, inside the cube)
    // the corners lie in one cell of level l on every axis while (lo ^ hi) >> (src_depth - l) == 0
    const uint32_t differ = uint32_t(b.lo[0] ^ b.hi[0]) | uint32_t(b.lo[1] ^ b.hi[1]) | uint32_t(b.lo[2] ^ b.hi[2]);
    const uint32_t last = t.src_depth - min(t.src_depth, bits_of(differ));
    while (m < last && src_interior(w)) {
        if (!src_step(src, t.src_words, w, child_of(b.lo[0], b.lo[1], b.lo[2], t.src_depth - m - 1u), status)) return;
        m++;
    }
}

// What the items of a frontier word come to, taken together: nothing (kOut), the value b (kLeaf) or a subtree (kNode); and
// whether an interior item's pointer is malformed, which matters once the word is opened or split.
struct Source {
    uint32_t kind, b, unaligned, outside;
};
__device__ inline Source frontier_source(const uint32_t *__restrict__ src, const Facing &t, const Box &b, uint32_t hint, uint32_t hint_level,
                                         uint32_t *status) {
    // normalised: OUT is the constant 0 where f(a, 0) = a; where f only asks whether b is set, every b != 0 is one value
    const bool out_is_zero = t.op <= SVO_COMBINE_CARVE, one_value = t.op == SVO_COMBINE_CARVE || t.op == SVO_COMBINE_KEEP;
    Source q = {kOut, 0u, 0u, 0u};
    const uint32_t e = uint32_t(max(max(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1]), b.hi[2] - b.lo[2])) + 1u;
    const uint32_t s_free = e == 1u ? 0u : bits_of(e - 1u);
    if (s_free > t.src_depth) {
        // a box larger than the cube: of the cells of the cube's size that it meets, the one at the origin is the root, an
        // interior word, and at least one other is OUT
        const int32_t side = int32_t(1u << t.src_depth);
        const bool root = b.lo[0] < side && b.hi[0] >= 0 && b.lo[1] < side && b.hi[1] >= 0 && b.lo[2] < side && b.hi[2] >= 0;
        if (root) q.kind = kNode;
        else if (out_is_zero) q.kind = kLeaf;
        return q;
    }
    const uint32_t s = s_free, k = t.src_depth - s;
    uint32_t w = hint, m = hint_level;
    shared_walk(src, t, b, w, m, status);
    const int32_t lx = b.lo[0] >> s, ly = b.lo[1] >> s, lz = b.lo[2] >> s;
    const uint32_t two = uint32_t((b.hi[0] >> s) != lx) << 2 | uint32_t((b.hi[1] >> s) != ly) << 1 | uint32_t((b.hi[2] >> s) != lz);
    const int32_t cells = int32_t(1u << k);
    uint32_t outs = 0, nodes = 0, constants = 0, value = 0, differ = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        if (j & ~two) continue;
        const int32_t ix = lx + int32_t(j >> 2), iy = ly + int32_t((j >> 1) & 1u), iz = lz + int32_t(j & 1u);
        uint32_t v = 0;
        if ((ix | iy | iz) < 0 || ix >= cells || iy >= cells || iz >= cells) {
            if (!out_is_zero) {
                outs++;
                continue;
            }
        } else {
            uint32_t item = w;
            bool whole = true;
            for (uint32_t l = m; l < k && src_interior(item) && whole; l++) whole = src_step(src, t.src_words, item, child_of(ix, iy, iz, k - l - 1u), status);
            if (!whole || src_interior(item)) {  // (a malformed pointer: the call is refused whatever the lane makes of it)
                nodes++;
                const uint32_t pointer = item >> 4;
                if (pointer & 7u) q.unaligned = 1u;
                else if (pointer + 8u > t.src_words) q.outside = 1u;
                continue;
            }
            v = (item >> 4) - SVO_VOXEL_OFFSET;
            if (one_value) v = v != 0u;
        }
        if (constants) differ |= uint32_t(v != value);
        else value = v;
        constants++;
    }
    if (nodes || differ || (outs && constants)) q.kind = kNode;
    else if (constants) q.kind = kLeaf, q.b = value;
    return q;
}

// The first frontier: the scene's root group, real, its parent the cell 0, whose box starts its walks at the source's root.
__global__ __launch_bounds__(64) void transform_root_kernel(uint32_t *__restrict__ gbase, uint64_t *__restrict__ gkey, uint32_t *__restrict__ gvirt,
                                                            uint32_t *__restrict__ ghint) {
    if (threadIdx.x == 0) gbase[0] = 0u, gvirt[0] = 0u, gkey[0] = 0ull, ghint[0] = 0u, ghint[1] = 0u;
}

// The rule for the frontier words of a level: svo_combine.hip's combine_plan_kernel behind the items.
__global__ __launch_bounds__(kThreads) void transform_plan_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Facing t, uint32_t level,
                                                                  Frontier f, const uint32_t *__restrict__ ghint, PlanOut o, uint32_t *status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < f.n) {
        const Entry e = frontier_entry(words, f, i);
        const Box box = word_box(t, e.x, e.y, e.z);
        const Source q = frontier_source(src, t, box, ghint[2u * (i >> 3)], ghint[2u * (i >> 3) + 1u], status);
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        const uint32_t a = leaf ? (e.word >> 4) - SVO_VOXEL_OFFSET : 0u;
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (q.kind == kLeaf) {
            if (leaf) {
                const uint32_t v = combine_value(t.op, a, q.b);
                if (v != a) at = e.at, out = leaf_word(v);
            } else {
                const uint32_t whole = whole_subtree(t.op, q.b != 0u);
                if (whole == kConstant) at = e.at, out = leaf_word(whole_constant(t.op, q.b));  // collapse
                else if (whole == kOpenIt) cd = level == t.depth ? kSceneFiner : kOpen;
            }
        } else if (q.kind == kNode) {
            if (!leaf) cd = level == t.depth ? kSceneFiner | kSourceFiner : kOpen;
            else if (!leaf_stays(t.op, a != 0u)) {
                if (level == t.depth) cd = kSourceFiner;
                else cd = kOpen | kSplit, at = e.at, fill = e.word & ~15u;
            }
        }
        if (cd & kOpen) {  // the source pointers that the next level starts from
            if (q.unaligned) status[kStSrcAlign] = 1u;
            if (q.outside) status[kStSrcRange] = 1u;
        }
        if (cd & (kSceneFiner | kSourceFiner)) refused = i;
        plan_store(o, i, cd, at, out, fill);
    }
    plan_refused(o, refused);
}

// Behind the two scans: the records of the next frontier's groups, each with the hint of its parent's box.
__global__ __launch_bounds__(kThreads) void transform_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Facing t, Frontier f,
                                                                  const uint32_t *__restrict__ ghint, EmitArgs a, uint32_t *__restrict__ next_hint) {
    Opened o;
    if (!emit_head(words, f, a, o)) return;
    const Box box = word_box(t, o.e.x, o.e.y, o.e.z);
    uint32_t w = ghint[2u * (o.i >> 3)], m = ghint[2u * (o.i >> 3) + 1u];
    shared_walk(src, t, box, w, m, a.status);
    next_hint[2u * o.k] = w;
    next_hint[2u * o.k + 1u] = m;
    emit_record(a, o);
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// What the transform keeps per context beside the walk's workspace (svo_ctx::transform): the hint per group of the two sets
// of frontier records, two u32 each, and the times.
struct svo_transform_state {
    svo_dev<uint32_t> ghint[2];
    svo_pass_timer<kEvs, SVO_TRANSFORM_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return SVO_OK;
    }
};

extern "C" {

int svo_nodes_transform(svo_ctx *ctx, const uint32_t *src_dev, const svo_transform_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (!src_dev) return svo_fail(ctx, SVO_ERR_ARG, "null source");
    if (p->op > SVO_COMBINE_REPLACE) return svo_fail(ctx, SVO_ERR_ARG, "op must be 0..5 (got " + std::to_string(p->op) + ")");
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (p->src_depth < 1 || p->src_depth > 21) return svo_fail(ctx, SVO_ERR_ARG, "src_depth must be 1..21 (got " + std::to_string(p->src_depth) + ")");
    for (int a = 0; a < 9; a++)
        if (p->matrix[a] < -kMaxEntry || p->matrix[a] > kMaxEntry)
            return svo_fail(ctx, SVO_ERR_ARG, "a matrix entry must lie in [-2^20, 2^20] (entry " + std::to_string(a) + ": " + std::to_string(p->matrix[a]) + ")");
    for (int a = 0; a < 3; a++)
        if (p->translate[a] < -kMaxTranslate || p->translate[a] > kMaxTranslate)
            return svo_fail(ctx, SVO_ERR_ARG, "a translation must lie in [-2^40, 2^40] (axis " + std::to_string(a) + ": " + std::to_string(p->translate[a]) + ")");
    if ((rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a transform cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    if (p->src_words < 8 || p->src_words % 8 || p->src_words > kMaxWords)
        return svo_fail(ctx, SVO_ERR_ARG, "src_words must be a positive multiple of 8, at most 2^27 (got " + std::to_string(p->src_words) + ")");
    if (src_dev < ctx->nodes + ctx->capacity && ctx->nodes < src_dev + p->src_words)
        return svo_fail(ctx, SVO_ERR_ARG, "the source overlaps the node buffer: the scene is edited in place, so the source must be a buffer of its own");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->transform))) return rc;
    svo_transform_state *s = ctx->transform.get();
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t depth = p->depth;
    struct : SourcePass {
        svo_transform_state *s;
        const uint32_t *src;
        Facing facing;
        int64_t spread[3];  // sum_j |matrix[i][j]|
        int grow(svo_ctx *ctx, int set, size_t groups) { return svo_grow(ctx, 2 * groups, &s->ghint[set]); }
        int root(svo_ctx *ctx, svo_frontier_walk &w) {
            transform_root_kernel<<<1, 64, 0, ctx->stream>>>(w.gbase[0], w.gkey[0], w.gvirt[0], s->ghint[0]);
            return SVO_OK;
        }
        void plan(svo_ctx *ctx, const Level &l) {
            facing.zc = 1u << (facing.depth - l.level);
            for (int a = 0; a < 3; a++) facing.rad[a] = int64_t(facing.zc - 1u) * spread[a];
            transform_plan_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src, facing, l.level, l.at, s->ghint[l.cur], l.out, l.emit.status);
        }
        void emit(svo_ctx *ctx, const Level &l) {  // (behind the level's plan: with its facing)
            transform_emit_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src, facing, l.at, s->ghint[l.cur], l.emit, s->ghint[l.nx]);
        }
    } pass;
    pass.src_words = p->src_words, pass.s = s, pass.src = src_dev;
    pass.facing = {};
    pass.facing.op = p->op, pass.facing.depth = depth, pass.facing.src_depth = p->src_depth, pass.facing.src_words = (uint32_t)p->src_words;
    for (int a = 0; a < 9; a++) pass.facing.m[a] = p->matrix[a];
    for (int a = 0; a < 3; a++) {
        pass.facing.t2[a] = 2 * p->translate[a];
        pass.spread[a] = std::abs(int64_t(p->matrix[3 * a])) + std::abs(int64_t(p->matrix[3 * a + 1])) + std::abs(int64_t(p->matrix[3 * a + 2]));
    }
    Walk walk;
    if ((rc = walk.begin(ctx, p->n_words, depth, "combined", s->timer.ev[kEvStart])) ||
        (rc = walk.run(ctx, pass, s->timer.ev[kEvPlan], s->timer.ev[kEvStatus])))
        return rc;
    if (walk.refused)  // from the refused word's flags, which tree goes on below it
        return svo_fail(ctx, SVO_ERR_STATE, std::string(kOpNames[p->op]) + " meets cell (" + std::to_string(walk.cell.x) + ", " + std::to_string(walk.cell.y) +
                                                ", " + std::to_string(walk.cell.z) + "), where " + finer_trees(walk.code) + " at depth " +
                                                std::to_string(depth) + ": finer there than the transform, which does not replace the subtree");
    if ((rc = walk.commit(ctx, p->max_words, s->timer.ev[kEvFill], s->timer.ev[kEvEnd], n_words_out))) return rc;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_transform_timing(svo_ctx *ctx, float ms_out[SVO_TRANSFORM_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->transform) return svo_fail(ctx, SVO_ERR_STATE, "no tree transformed on this context yet");
    return ctx->transform->timer.read(ctx, ms_out);
}

}  // extern "C"

// svo_place.hip -- a tree placed into the scene at any cell offset and in any of the cube's 48 orientations: the
// combine of two trees (svo_combine.hip) without the condition that the source's cube is a cell of the scene's
// octree.  include/svo_hip.h has the rule for one word; this file applies it level by level with the walk of svo_frontier.h
//  and the combine's plan.  One thing differs: a scene word of a level faces not one source word but the up to
// 2 x 2 x 2 cells of its own size of the oriented source that its cube overlaps, its *items*.
//
//   items     one word each: OUT, a source word without its counter (a leaf: a constant, carried down as it is; an interior
//             word: a source group) or ABOVE k, the cell of size S 2^k at the origin of the source's grid, k >= 1, which holds
//             the source's cube in its corner: a word faces it only when its own cube overlaps the source's, else it is OUT.  A
//             frontier group's record holds, beside the scene's side as in svo_combine.hip, the eight items of its parent's
//             cell, 32 bytes, at jx << 2 | jy << 1 | jz; an axis with one cell leaves j = 1 unused (OUT)
//   level     which item of the parent a child's item j is a child of, and which child, is the same for every word of a
//             level: per axis t = c + h + j, the parent's item t >> 1, its child t & 1, with h = ((-offset) mod 2 z) >= z and
//             j <= two = ((-offset) mod z != 0).  The host computes h and two per level and passes them by value; a lane reads
//             its parent's items from the record by that index
//   orient    an oriented child index becomes the source's by one table of eight (bit i of the oriented index is bit perm[i]
//             of the source's, flipped with f_i), the same at every level; above the root nothing is turned, the oriented
//             source lies at the origin whatever the orientation
//   plan      per level, reading only, one lane per frontier word: its items taken together (normalised as the header says)
//             are nothing (all OUT), one constant or a subtree, and from there on the lane is the combine's
//   emit      a followed source pointer is every interior item of a word that is opened or split
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_combine_rules.h"  // (combine_value, whole_subtree, whole_constant, leaf_stays; Src, kSceneFiner, kSourceFiner, kOpNames, SourcePass)
#include "svo_ctx.h"
#include "svo_frontier.h"  // (the walk: Entry, PlanOut, emit_head, Walk; kNone, leaf_word)

namespace {

constexpr int64_t kMaxOffset = int64_t(1) << 21;
// an item's low four bits: 0 = a source word without its counter; kItemOut; kItemAbove, with k in the bits above
constexpr uint32_t kItemOut = 1u, kItemAbove = 2u;
// The call's constants and the level's, by value to the kernels.  child_map: three bits per oriented child index, the source's
// child index.  side: S.  cell: the level's z; h, two: its remainders, x << 2 | y << 1 | z.
struct Facing {
    uint32_t op, depth, child_map, side;
    int32_t offset[3];
    uint32_t cell, h, two;
};

// Item j (a subset of t.two's bits) of child c, the word of the level's cell (x, y, z), of the group g: the child of one of the
// eight items in the group's record.  An interior item's pointer passed the emit's check, pointer + 8 <= src_words, before this
// level was planned.
__device__ inline uint32_t child_item(const uint32_t *__restrict__ src, const uint32_t *__restrict__ gitem, const Facing &t, uint32_t g, uint32_t c,
                                      uint32_t j, uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t tx = (c >> 2) + (t.h >> 2) + (j >> 2), ty = ((c >> 1) & 1u) + ((t.h >> 1) & 1u) + ((j >> 1) & 1u), tz = (c & 1u) + (t.h & 1u) + (j & 1u);
    const uint32_t slot = (tx >> 1) << 2 | (ty >> 1) << 1 | tz >> 1, child = (tx & 1u) << 2 | (ty & 1u) << 1 | (tz & 1u);
    const uint32_t parent = gitem[8u * g + slot], tag = parent & 15u;
    if (tag == kItemOut) return kItemOut;
    if (tag == kItemAbove) {  // the child at the origin leads on, to the source's root in the end: an interior word pointing at group 0
        if (child) return kItemOut;
        const uint32_t k = parent >> 4;
        if (k == 1u) return 0u;
        // a cell above the root holds the source's cube in its corner [0, S)^3 and nothing else: a word beside that is OUT of it
        const int32_t side = int32_t(t.side), cell = int32_t(t.cell);
        if (int32_t(x) * cell - t.offset[0] >= side || int32_t(y) * cell - t.offset[1] >= side || int32_t(z) * cell - t.offset[2] >= side) return kItemOut;
        return (k - 1u) << 4 | kItemAbove;
    }
    if ((parent >> 4) >= SVO_VOXEL_OFFSET) return parent;  // a constant, carried down
    return src[(parent >> 4) + (t.child_map >> (3u * child) & 7u)] & ~15u;
}

// What the items of frontier word i, whose entry is e, come to, taken together: nothing (kOut), the value b (kLeaf) or a
// subtree (kNode).
struct Source {
    uint32_t kind, b;
};
__device__ inline Source frontier_source(const uint32_t *__restrict__ src, const Facing &t, const uint32_t *__restrict__ gitem, uint32_t i, const Entry &e) {
    const uint32_t g = i >> 3, c = i & 7u;
    // normalised: OUT is the constant 0 where f(a, 0) = a; where f only asks whether b is set, every b != 0 is one value
    const bool out_is_zero = t.op <= SVO_COMBINE_CARVE, one_value = t.op == SVO_COMBINE_CARVE || t.op == SVO_COMBINE_KEEP;
    uint32_t outs = 0, nodes = 0, constants = 0, value = 0, differ = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        if (j & ~t.two) continue;  // (the same for the whole launch)
        const uint32_t item = child_item(src, gitem, t, g, c, j, e.x, e.y, e.z), tag = item & 15u, field = item >> 4;
        uint32_t v = 0;
        if (tag == kItemOut) {
            if (!out_is_zero) {
                outs++;
                continue;
            }
        } else if (tag == kItemAbove || field < SVO_VOXEL_OFFSET) {
            nodes++;
            continue;
        } else {
            v = field - SVO_VOXEL_OFFSET;
            if (one_value) v = v != 0u;
        }
        if (constants) differ |= uint32_t(v != value);
        else value = v;
        constants++;
    }
    Source q = {kOut, 0u};
    if (nodes || differ || (outs && constants)) q.kind = kNode;
    else if (constants) q.kind = kLeaf, q.b = value;
    return q;
}

// The first frontier: the scene's root group, real, its parent the cell 0, whose items are OUT but for the one (if any) that
// holds the source's cube.
__global__ __launch_bounds__(8) void place_root_kernel(uint32_t *__restrict__ gbase, uint64_t *__restrict__ gkey, uint32_t *__restrict__ gvirt,
                                                       uint32_t *__restrict__ gitem, uint32_t live, uint32_t item) {
    const uint32_t j = threadIdx.x;
    if (j == 0) gbase[0] = 0u, gvirt[0] = 0u, gkey[0] = 0ull;
    if (j < 8u) gitem[j] = j == live ? item : kItemOut;
}

// The rule for the frontier words of a level: svo_combine.hip's combine_plan_kernel behind the items.
__global__ __launch_bounds__(kThreads) void place_plan_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Facing t, uint32_t level,
                                                              Frontier f, const uint32_t *__restrict__ gitem, PlanOut o) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < f.n) {
        const Entry e = frontier_entry(words, f, i);
        const Source q = frontier_source(src, t, gitem, i, e);
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
        if (cd & (kSceneFiner | kSourceFiner)) refused = i;
        plan_store(o, i, cd, at, out, fill);
    }
    plan_refused(o, refused);
}

// Behind the two scans: the records of the next frontier's groups with their eight items.  A source pointer that is followed,
// every interior item's, is checked as the discovery checks it.
__global__ __launch_bounds__(kThreads) void place_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Facing t, Frontier f,
                                                              const uint32_t *__restrict__ gitem, EmitArgs a, uint32_t src_words,
                                                              uint32_t *__restrict__ next_item) {
    Opened o;
    if (!emit_head(words, f, a, o)) return;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        uint32_t item = kItemOut;
        if (!(j & ~t.two)) {
            item = child_item(src, gitem, t, o.i >> 3, o.i & 7u, j, o.e.x, o.e.y, o.e.z);
            if (!(item & 15u) && (item >> 4) < SVO_VOXEL_OFFSET) {
                if ((item >> 4) & 7u) a.status[kStSrcAlign] = 1u;
                else if (uint64_t(item >> 4) + 8u > src_words) a.status[kStSrcRange] = 1u;
            }
        }
        next_item[8u * o.k + j] = item;
    }
    emit_record(a, o);
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

// (-offset) mod m, m a power of two
inline uint32_t minus_mod(int32_t offset, uint32_t m) { return uint32_t(-int64_t(offset)) & (m - 1u); }

}  // namespace

// What the placement keeps per context beside the walk's workspace (svo_ctx::place): the eight items per group of the two
// sets of frontier records, and the times.
struct svo_place_state {
    svo_dev<uint32_t> gitem[2];
    svo_pass_timer<kEvs, SVO_PLACE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return SVO_OK;
    }
};

namespace {

const uint8_t kPerms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// three bits per oriented child index r: the source's child index q, bit of q[perm[i]] = bit of r[i] ^ f_i
uint32_t child_map_of(uint32_t orient) {
    const uint8_t *perm = kPerms[orient >> 3];
    uint32_t map = 0;
    for (uint32_t r = 0; r < 8; r++) {
        uint32_t q = 0;
        for (uint32_t i = 0; i < 3; i++) {
            const uint32_t bit = ((r >> (2 - i)) ^ (orient >> (2 - i))) & 1u;
            q |= bit << (2 - perm[i]);
        }
        map |= q << (3 * r);
    }
    return map;
}

}  // namespace

extern "C" {

int svo_nodes_place(svo_ctx *ctx, const uint32_t *src_dev, const svo_place_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (!src_dev) return svo_fail(ctx, SVO_ERR_ARG, "null source");
    if (p->op > SVO_COMBINE_REPLACE) return svo_fail(ctx, SVO_ERR_ARG, "op must be 0..5 (got " + std::to_string(p->op) + ")");
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (p->src_depth < 1 || p->src_depth > p->depth)
        return svo_fail(ctx, SVO_ERR_ARG, "src_depth must be 1..depth (got " + std::to_string(p->src_depth) + ", depth " + std::to_string(p->depth) + ")");
    if (p->orient >= SVO_PLACE_ORIENTS) return svo_fail(ctx, SVO_ERR_ARG, "orient must be 0..47 (got " + std::to_string(p->orient) + ")");
    for (int a = 0; a < 3; a++)
        if (p->offset[a] < -kMaxOffset || p->offset[a] > kMaxOffset)
            return svo_fail(ctx, SVO_ERR_ARG, "offset must lie in [-2^21, 2^21] on every axis (axis " + std::to_string(a) + ": " + std::to_string(p->offset[a]) + ")");
    if ((rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a placement cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    if (p->src_words < 8 || p->src_words % 8 || p->src_words > kMaxWords)
        return svo_fail(ctx, SVO_ERR_ARG, "src_words must be a positive multiple of 8, at most 2^27 (got " + std::to_string(p->src_words) + ")");
    if (src_dev < ctx->nodes + ctx->capacity && ctx->nodes < src_dev + p->src_words)
        return svo_fail(ctx, SVO_ERR_ARG, "the source overlaps the node buffer: the scene is edited in place, so the source must be a buffer of its own");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->place))) return rc;
    svo_place_state *s = ctx->place.get();
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t depth = p->depth;
    // the root group's record: of the items of the whole scene cube, cells of 2^depth >= S, the one at the origin of the
    // source's grid holds the source's cube: ABOVE depth - src_depth, or the root itself
    uint32_t live = 0;  // its index in the record; 8: none, the source lies wholly outside
    for (int a = 0; a < 3; a++) {
        const int64_t first = -int64_t(p->offset[a]) >> depth;  // floor((-offset) / 2^depth): the axis' first cell, and the next when there are two
        const bool two = minus_mod(p->offset[a], 1u << depth) != 0u;
        if (first == -1 && two) live |= 4u >> a;
        else if (first != 0) live |= 8u;
    }
    live = std::min(live, 8u);
    struct : SourcePass {
        svo_place_state *s;
        const uint32_t *src;
        const svo_place_params *p;
        Facing facing;
        uint32_t live, above;
        int grow(svo_ctx *ctx, int set, size_t groups) { return svo_grow(ctx, 8 * groups, &s->gitem[set]); }
        int root(svo_ctx *ctx, svo_frontier_walk &w) {
            place_root_kernel<<<1, 8, 0, ctx->stream>>>(w.gbase[0], w.gkey[0], w.gvirt[0], s->gitem[0], live, above ? above << 4 | kItemAbove : 0u);
            return SVO_OK;
        }
        void plan(svo_ctx *ctx, const Level &l) {
            const uint32_t z = 1u << (facing.depth - l.level);
            facing.cell = z, facing.h = facing.two = 0;
            for (int a = 0; a < 3; a++) {
                const uint32_t rem = minus_mod(p->offset[a], 2u * z);
                facing.h |= uint32_t(rem >= z) << (2 - a);
                facing.two |= uint32_t((rem & (z - 1u)) != 0u) << (2 - a);
            }
            place_plan_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src, facing, l.level, l.at, s->gitem[l.cur], l.out);
        }
        void emit(svo_ctx *ctx, const Level &l) {  // (behind the level's plan: with its facing)
            place_emit_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src, facing, l.at, s->gitem[l.cur], l.emit, (uint32_t)src_words,
                                                                   s->gitem[l.nx]);
        }
    } pass;
    pass.src_words = p->src_words, pass.s = s, pass.src = src_dev, pass.p = p, pass.live = live, pass.above = depth - p->src_depth;
    pass.facing = {p->op, depth, child_map_of(p->orient), 1u << p->src_depth, {p->offset[0], p->offset[1], p->offset[2]}, 0u, 0u, 0u};
    Walk walk;
    if ((rc = walk.begin(ctx, p->n_words, depth, "combined", s->timer.ev[kEvStart])) ||
        (rc = walk.run(ctx, pass, s->timer.ev[kEvPlan], s->timer.ev[kEvStatus])))
        return rc;
    if (walk.refused)  // from the refused word's flags, which tree goes on below it
        return svo_fail(ctx, SVO_ERR_STATE, std::string(kOpNames[p->op]) + " meets cell (" + std::to_string(walk.cell.x) + ", " + std::to_string(walk.cell.y) +
                                                ", " + std::to_string(walk.cell.z) + "), where " + finer_trees(walk.code) + " at depth " +
                                                std::to_string(depth) + ": finer there than the placement, which does not replace the subtree");
    if ((rc = walk.commit(ctx, p->max_words, s->timer.ev[kEvFill], s->timer.ev[kEvEnd], n_words_out))) return rc;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_place_timing(svo_ctx *ctx, float ms_out[SVO_PLACE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->place) return svo_fail(ctx, SVO_ERR_STATE, "no tree placed on this context yet");
    return ctx->place->timer.read(ctx, ms_out);
}

}  // extern "C"

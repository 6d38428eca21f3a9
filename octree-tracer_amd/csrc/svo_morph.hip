// svo_morph.hip -- one step of mathematical morphology on the tree in the node buffer: grow it by the cells
// that touch a voxel, or shrink it by the voxels that touch an empty cell, under 6, 18 or 26 neighbours.  include/svo_hip.h has
// the rule for one cell and for one word; this file applies it level by level with the walk of svo_frontier.h.
// Where a placed scene word (svo_place.hip) faces up to 2 x 2 x 2 cells of a second tree, a word here faces the 3 x 3 x 3
// cells of its own level of the scene itself: the plan never writes, so the tree is its own neighbour as it was before the
// call.
//
//   items     one word each: OUT (outside the grid) or a scene word without its counter (a leaf: a constant, carried down as
//             it is; an interior word: a group of the scene).  A frontier group's record holds, beside the scene's side as in
//             svo_combine.hip, the 27 items of its parent's cell, the cell itself among them, at 9 (ex + 1) + 3 (ey + 1) + ez + 1;
//             those that the call's conn never reads (edges and corners under 6, corners under 18) are not written
//   level     item d of child c is, per axis with t = c + d in -1..2, the child t & 1 of the parent's item floor(t / 2): a
//             lane reads the parent's item from the record by that index and, when it is interior, the child from the words
//   plan      per level, reading only, one lane per frontier word.  An interior word is opened; a leaf that the op cannot
//             change is done; any other leaf folds its counting items, in the order of the per-cell rule, into three numbers
//             (not quiet, interior among those, the first value set) and is left, overwritten, split or refused by them
//   emit      a pointer that a later level follows is every interior item written into a record, checked where it is written
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_frontier.h"  // (the walk: Entry, PlanOut, emit_head, Walk; kNone, leaf_word)

namespace {

constexpr uint32_t kItems = 27, kCentre = 13;
constexpr uint32_t kItemOut = 1u;  // an item's low four bits: 0 = a scene word without its counter
// a word's flag above the walk's: an interior word at level `depth`, or a leaf there that an interior item would change
constexpr uint32_t kFiner = 4u;

// The call's constants, by value to the kernels.  reach: 1, 2 or 3, the largest |d|_1 of conn's offsets.
struct Morph {
    uint32_t op, reach, depth, open_boundary, colour;
};

// Item (dx, dy, dz) of child c of the group g: the child of one of the 27 items in the group's record.  An interior item's
// pointer passed the emit's check, pointer + 8 <= n_words, before this level was planned.
__device__ inline uint32_t child_item(const uint32_t *__restrict__ words, const uint32_t *__restrict__ gitem, uint32_t g, uint32_t c, int dx, int dy,
                                      int dz) {
    const int tx = int(c >> 2) + dx, ty = int((c >> 1) & 1u) + dy, tz = int(c & 1u) + dz;
    const uint32_t slot = uint32_t(9 * ((tx >> 1) + 1) + 3 * ((ty >> 1) + 1) + (tz >> 1) + 1);
    const uint32_t parent = gitem[size_t(kItems) * g + slot];
    if (parent == kItemOut || (parent >> 4) >= SVO_VOXEL_OFFSET) return parent;  // OUT, or a constant carried down
    return words[(parent >> 4) + uint32_t((tx & 1) << 2 | (ty & 1) << 1 | (tz & 1))] & ~15u;
}

// The first frontier: the scene's root group, real, its parent the cell 0 of level 0, the whole grid, as an interior word
// pointing at group 0, with OUT on every side.
__global__ __launch_bounds__(32) void morph_root_kernel(uint32_t *__restrict__ gbase, uint64_t *__restrict__ gkey, uint32_t *__restrict__ gvirt,
                                                        uint32_t *__restrict__ gitem) {
    const uint32_t j = threadIdx.x;
    if (j == 0) gbase[0] = 0u, gvirt[0] = 0u, gkey[0] = 0ull;
    if (j < kItems) gitem[j] = j == kCentre ? 0u : kItemOut;
}

// The rule for the frontier words of a level.
__global__ __launch_bounds__(kThreads) void morph_plan_kernel(const uint32_t *__restrict__ words, Morph m, uint32_t level, Frontier f,
                                                              const uint32_t *__restrict__ gitem, PlanOut o) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < f.n) {
        const uint32_t g = i >> 3, c = i & 7u;
        const Entry e = frontier_entry(words, f, i);
        const uint32_t here = e.at, word = e.word;
        const bool grow = m.op == SVO_MORPH_GROW;
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if ((word >> 4) < SVO_VOXEL_OFFSET) cd = level == m.depth ? kFiner : kOpen;
        else if (((word >> 4) != SVO_VOXEL_OFFSET) != grow) {  // a leaf that the op can change: an empty one grows, a voxel shrinks
            // normalised: OUT is the constant 0 for a grow, and for a shrink a value that is set, or 0 under an open boundary
            const uint32_t out_item = grow || m.open_boundary ? leaf_word(0u) : leaf_word(1u);
            uint32_t loud = 0, nodes = 0, first = 0;
#pragma unroll
            for (int norm = 1; norm <= 3; norm++) {
                if (uint32_t(norm) > m.reach) continue;  // (the same for the whole launch)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dz = -1; dz <= 1; dz++) {
                            if ((dx != 0) + (dy != 0) + (dz != 0) != norm) continue;  // (folded away: the offsets in priority order)
                            uint32_t item = child_item(words, gitem, g, c, dx, dy, dz);
                            if (item == kItemOut) item = out_item;
                            const uint32_t field = item >> 4;
                            if (field < SVO_VOXEL_OFFSET) loud++, nodes++;
                            else if ((field != SVO_VOXEL_OFFSET) == grow) {
                                loud++;
                                if (!first) first = field - SVO_VOXEL_OFFSET;
                            }
                        }
            }
            if (loud) {
                if (level < m.depth) cd = kOpen | kSplit, at = here, fill = word & ~15u;
                else if (nodes) cd = kFiner;
                else at = here, out = leaf_word(grow ? (m.colour ? m.colour : first) : 0u);
            }
        }
        if (cd & kFiner) refused = i;
        plan_store(o, i, cd, at, out, fill);
    }
    plan_refused(o, refused);
}

// Behind the two scans: the records of the next frontier's groups with their items.  A pointer that is followed is checked
// as the discovery checks it: the word's own by emit_head, and every interior item's here.  (The centre item of an opened
// word of a real group is that word, so its pointer is checked twice, to the same end.)
__global__ __launch_bounds__(kThreads) void morph_emit_kernel(const uint32_t *__restrict__ words, Morph m, Frontier f, const uint32_t *__restrict__ gitem,
                                                              EmitArgs a, uint32_t *__restrict__ next_item) {
    Opened o;
    if (!emit_head(words, f, a, o)) return;
    // the word's cell and its neighbours: the cell itself is the word, a split's the constant it hands down
#pragma unroll
    for (int dx = -1; dx <= 1; dx++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dz = -1; dz <= 1; dz++) {
                if (uint32_t((dx != 0) + (dy != 0) + (dz != 0)) > m.reach) continue;  // (the same for the whole launch)
                const uint32_t item = child_item(words, gitem, o.i >> 3, o.i & 7u, dx, dy, dz);
                if (item != kItemOut && (item >> 4) < SVO_VOXEL_OFFSET) {
                    if ((item >> 4) & 7u) a.status[kStAlign] = 1u;  // (every writer stores the same value)
                    else if (uint64_t(item >> 4) + 8u > a.n_words) a.status[kStRange] = 1u;
                }
                next_item[size_t(kItems) * o.k + uint32_t(9 * (dx + 1) + 3 * (dy + 1) + dz + 1)] = item;
            }
    emit_record(a, o);
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// What the morphology keeps per context beside the walk's workspace (svo_ctx::morph): the 27 items per group of the two
// sets of frontier records, and the times.
struct svo_morph_state {
    svo_dev<uint32_t> gitem[2];
    svo_pass_timer<kEvs, SVO_MORPH_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return SVO_OK;
    }
};

namespace {

const char *const kOpNames[] = {"grow", "shrink"};

}  // namespace

extern "C" {

int svo_nodes_morph(svo_ctx *ctx, const svo_morph_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (p->op > SVO_MORPH_SHRINK) return svo_fail(ctx, SVO_ERR_ARG, "op must be 0 or 1 (got " + std::to_string(p->op) + ")");
    if (p->conn != 6 && p->conn != 18 && p->conn != 26) return svo_fail(ctx, SVO_ERR_ARG, "conn must be 6, 18 or 26 (got " + std::to_string(p->conn) + ")");
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (p->flags & ~SVO_MORPH_OPEN_BOUNDARY) return svo_fail(ctx, SVO_ERR_ARG, "unknown flag bits (got " + std::to_string(p->flags) + ")");
    if (p->op == SVO_MORPH_SHRINK && p->colour) return svo_fail(ctx, SVO_ERR_ARG, "a shrink makes no cells: colour must be 0");
    if ((rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a morphology step splits leaves under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->morph))) return rc;
    svo_morph_state *s = ctx->morph.get();
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t depth = p->depth;
    struct : FrontierPass {
        svo_morph_state *s;
        Morph morph;
        int grow(svo_ctx *ctx, int set, size_t groups) { return svo_grow(ctx, kItems * groups, &s->gitem[set]); }
        int root(svo_ctx *ctx, svo_frontier_walk &w) {
            morph_root_kernel<<<1, 32, 0, ctx->stream>>>(w.gbase[0], w.gkey[0], w.gvirt[0], s->gitem[0]);
            return SVO_OK;
        }
        void plan(svo_ctx *ctx, const Level &l) {
            morph_plan_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, morph, l.level, l.at, s->gitem[l.cur], l.out);
        }
        void emit(svo_ctx *ctx, const Level &l) {
            morph_emit_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, morph, l.at, s->gitem[l.cur], l.emit, s->gitem[l.nx]);
        }
    } pass;
    pass.s = s;
    pass.morph = {p->op, p->conn == 6 ? 1u : p->conn == 18 ? 2u : 3u, depth, p->flags & SVO_MORPH_OPEN_BOUNDARY, p->colour & 0xFFFFFFu};
    Walk walk;
    if ((rc = walk.begin(ctx, p->n_words, depth, "new", s->timer.ev[kEvStart])) || (rc = walk.run(ctx, pass, s->timer.ev[kEvPlan], s->timer.ev[kEvStatus])))
        return rc;
    if (walk.refused)
        return svo_fail(ctx, SVO_ERR_STATE, std::string(kOpNames[p->op]) + " meets cell (" + std::to_string(walk.cell.x) + ", " + std::to_string(walk.cell.y) +
                                                ", " + std::to_string(walk.cell.z) + "), where the tree is finer than depth " + std::to_string(depth) +
                                                ": the cell or a neighbour that would change it is an interior node there");
    if ((rc = walk.commit(ctx, p->max_words, s->timer.ev[kEvFill], s->timer.ev[kEvEnd], n_words_out))) return rc;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_morph_timing(svo_ctx *ctx, float ms_out[SVO_MORPH_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->morph) return svo_fail(ctx, SVO_ERR_STATE, "no morphology step run on this context yet");
    return ctx->morph->timer.read(ctx, ms_out);
}

}  // extern "C"

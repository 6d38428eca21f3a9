// svo_combine.hip -- two trees combined: the tree in the node buffer, the scene, edited in place by a second
// tree, the source, that is only read: pasted over it, filled under it, painted, carved, masked or put in its place, whole
// or into one cell of a coarser level.  include/svo_hip.h has the rule for one word; this file applies it level by level in
// svo_region.hip's frame, with a tree where that file has shapes.  Scans instead of atomics: the words do not depend on the
// run.
//
// The walk is svo_frontier.h's: frontier, scans, check, status and commit, none of which reads the source;
// this file has the source's side of a group's record, the plan, and the emit that hands the source down.
//
//   record    beside the walk's, one word of the source per group, read like a word of a tree: an interior field is the
//             source group whose eight words pair with the scene's by child index, a leaf field is a constant carried down
//             that all eight pair with, and kSrcPath in the counter's bits says that the group lies above the placement: one
//             child leads on towards the cell `at`, the other seven lie outside the source
//   plan      per level, reading only, one lane per frontier word: the eight lanes of a group read the scene's group and
//             the source's as one 32-byte line each.  The lane decides by a table over the op and whether either value is
//             empty
//   emit      a source pointer that is followed is checked as a scene pointer is.  A source group may be reached as often
//             as it likes: it is only read
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_combine_rules.h"  // (combine_value, whole_subtree, whole_constant, leaf_stays; Src, kSceneFiner, kSourceFiner, kOpNames, SourcePass)
#include "svo_ctx.h"
#include "svo_frontier.h"  // (the walk: Entry, PlanOut, emit_head, Walk; kNone, leaf_word)

namespace {

constexpr uint32_t kSrcPath = 8u;  // a group's source record: above the placement (no source word has it: the records' low four bits are 0)

// (the rule's tables over the op and whether either value is empty: svo_combine_rules.h, shared with svo_place.hip)

// The call's constants, by value to the kernels.
struct Placement {
    uint32_t op, depth, at_level, at[3];
};

// What the source has for the cube of frontier word i: nothing (kOut), the value b (kLeaf), or a subtree (kNode), whose
// children's record is `next`.
struct Source {
    uint32_t kind, b, next;
};
__device__ inline Source frontier_source(const uint32_t *__restrict__ src, const Placement &pl, uint32_t level, const uint32_t *__restrict__ gsrc,
                                         uint32_t i) {
    const uint32_t c = i & 7u, rec = gsrc[i >> 3];
    Source e;
    e.b = e.next = 0;
    if ((rec & 15u) == kSrcPath) {  // level <= at_level: the child towards `at` goes on, to the source's root in the end
        const uint32_t up = pl.at_level - level;
        const uint32_t live = ((pl.at[0] >> up) & 1u) << 2 | ((pl.at[1] >> up) & 1u) << 1 | ((pl.at[2] >> up) & 1u);
        e.kind = c == live ? kNode : kOut;
        e.next = up ? kSrcPath : 0u;
        return e;
    }
    // a constant's record is a leaf word itself; a group's pointer passed the check: pointer + 8 <= src_words
    const uint32_t field = (rec >> 4) >= SVO_VOXEL_OFFSET ? rec >> 4 : src[(rec >> 4) + c] >> 4;
    if (field >= SVO_VOXEL_OFFSET) e.kind = kLeaf, e.b = field - SVO_VOXEL_OFFSET;
    else e.kind = kNode, e.next = field << 4;
    return e;
}

// The rule for the frontier words of `level`; a word that would be opened or split at level == depth is refused.
__global__ __launch_bounds__(kThreads) void combine_plan_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Placement pl,
                                                                uint32_t level, Frontier f, const uint32_t *__restrict__ gsrc, PlanOut o) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < f.n) {
        const Entry e = frontier_entry(words, f, i);
        const Source q = frontier_source(src, pl, level, gsrc, i);
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        const uint32_t a = leaf ? (e.word >> 4) - SVO_VOXEL_OFFSET : 0u;
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (q.kind == kLeaf) {
            if (leaf) {
                const uint32_t v = combine_value(pl.op, a, q.b);
                if (v != a) at = e.at, out = leaf_word(v);
            } else {
                const uint32_t whole = whole_subtree(pl.op, q.b != 0u);
                if (whole == kConstant) at = e.at, out = leaf_word(whole_constant(pl.op, q.b));  // collapse
                else if (whole == kOpenIt) cd = level == pl.depth ? kSceneFiner : kOpen;
            }
        } else if (q.kind == kNode) {
            if (!leaf) cd = level == pl.depth ? kSceneFiner | kSourceFiner : kOpen;
            else if (!leaf_stays(pl.op, a != 0u)) {
                if (level == pl.depth) cd = kSourceFiner;
                else cd = kOpen | kSplit, at = e.at, fill = e.word & ~15u;
            }
        }
        if (cd & (kSceneFiner | kSourceFiner)) refused = i;
        plan_store(o, i, cd, at, out, fill);
    }
    plan_refused(o, refused);
}

// Behind the two scans: the records of the next frontier's groups with the source's side.  A source pointer that is
// followed is checked as the discovery checks it.
__global__ __launch_bounds__(kThreads) void combine_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Placement pl,
                                                                uint32_t level, Frontier f, const uint32_t *__restrict__ gsrc, EmitArgs a,
                                                                uint32_t src_words, uint32_t *__restrict__ next_src) {
    Opened o;
    if (!emit_head(words, f, a, o)) return;
    const Source q = frontier_source(src, pl, level, gsrc, o.i);
    uint32_t rec = q.next;
    if (q.kind == kLeaf) rec = leaf_word(q.b);  // the constant, carried down
    else if (rec != kSrcPath) {
        if ((rec >> 4) & 7u) a.status[kStSrcAlign] = 1u;
        else if (uint64_t(rec >> 4) + 8u > src_words) a.status[kStSrcRange] = 1u;
    }
    next_src[o.k] = rec;
    emit_record(a, o);
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// What the combine keeps per context beside the walk's workspace (svo_ctx::combine): the source's side of the two sets of
// frontier records, and the times.
struct svo_combine_state {
    svo_dev<uint32_t> gsrc[2];
    svo_pass_timer<kEvs, SVO_COMBINE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return SVO_OK;
    }
};

extern "C" {

int svo_nodes_combine(svo_ctx *ctx, const uint32_t *src_dev, const svo_combine_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (!src_dev) return svo_fail(ctx, SVO_ERR_ARG, "null source");
    if (p->op > SVO_COMBINE_REPLACE) return svo_fail(ctx, SVO_ERR_ARG, "op must be 0..5 (got " + std::to_string(p->op) + ")");
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (p->at_level >= p->depth)
        return svo_fail(ctx, SVO_ERR_ARG, "at_level must be below depth (got " + std::to_string(p->at_level) + ", depth " + std::to_string(p->depth) + ")");
    for (int a = 0; a < 3; a++)
        if (p->at[a] >> p->at_level)
            return svo_fail(ctx, SVO_ERR_ARG, "at must lie in [0, 2^at_level) on every axis (axis " + std::to_string(a) + ": " + std::to_string(p->at[a]) +
                                                  ", at_level " + std::to_string(p->at_level) + ")");
    if ((rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a combine cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    if (p->src_words < 8 || p->src_words % 8 || p->src_words > kMaxWords)
        return svo_fail(ctx, SVO_ERR_ARG, "src_words must be a positive multiple of 8, at most 2^27 (got " + std::to_string(p->src_words) + ")");
    if (src_dev < ctx->nodes + ctx->capacity && ctx->nodes < src_dev + p->src_words)
        return svo_fail(ctx, SVO_ERR_ARG, "the source overlaps the node buffer: the scene is edited in place, so the source must be a buffer of its own");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->combine))) return rc;
    svo_combine_state *s = ctx->combine.get();
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t depth = p->depth;
    struct : SourcePass {
        svo_combine_state *s;
        const uint32_t *src;
        const svo_combine_params *p;
        Placement pl;
        int grow(svo_ctx *ctx, int set, size_t groups) { return svo_grow(ctx, groups, &s->gsrc[set]); }
        // level 1: the scene's root group against the source's root group or the path to `at`
        int root(svo_ctx *ctx, svo_frontier_walk &w) {
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)s->gsrc[0].get(), p->at_level ? (int)kSrcPath : 0, 1, ctx->stream));
            return FrontierPass::root(ctx, w);
        }
        void plan(svo_ctx *ctx, const Level &l) {
            combine_plan_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src, pl, l.level, l.at, s->gsrc[l.cur], l.out);
        }
        void emit(svo_ctx *ctx, const Level &l) {
            combine_emit_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src, pl, l.level, l.at, s->gsrc[l.cur], l.emit, (uint32_t)src_words,
                                                                     s->gsrc[l.nx]);
        }
    } pass;
    pass.src_words = p->src_words, pass.s = s, pass.src = src_dev, pass.p = p, pass.pl = {p->op, depth, p->at_level, {p->at[0], p->at[1], p->at[2]}};
    Walk walk;
    if ((rc = walk.begin(ctx, p->n_words, depth, "combined", s->timer.ev[kEvStart])) ||
        (rc = walk.run(ctx, pass, s->timer.ev[kEvPlan], s->timer.ev[kEvStatus])))
        return rc;
    if (walk.refused)  // from the refused word's flags, which tree goes on below it
        return svo_fail(ctx, SVO_ERR_STATE, std::string(kOpNames[p->op]) + " meets cell (" + std::to_string(walk.cell.x) + ", " + std::to_string(walk.cell.y) +
                                                ", " + std::to_string(walk.cell.z) + "), where " + finer_trees(walk.code) + " at depth " +
                                                std::to_string(depth) + ": finer there than the combine, which does not replace the subtree");
    if ((rc = walk.commit(ctx, p->max_words, s->timer.ev[kEvFill], s->timer.ev[kEvEnd], n_words_out))) return rc;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_combine_timing(svo_ctx *ctx, float ms_out[SVO_COMBINE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->combine) return svo_fail(ctx, SVO_ERR_STATE, "no trees combined on this context yet");
    return ctx->combine->timer.read(ctx, ms_out);
}

}  // extern "C"

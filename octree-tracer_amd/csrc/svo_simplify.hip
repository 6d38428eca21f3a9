// svo_simplify.hip -- the tree in the node buffer simplified: SVO_SIMPLIFY_MERGE turns an interior word
// whose whole subtree holds one leaf value into that leaf, SVO_SIMPLIFY_CUT turns every interior word of one level into a
// leaf of its subtree's mip colour; the rest comes out in the compaction's canonical breadth-first layout, in place or
// into a buffer of the caller's.  The compaction's frame (svo_tree_rewrite, svo_compact.hip) and its 8 lanes per group
// (svo_group.h) with a reduce in the place of its prune:
//
//   begin     svo_tree_rewrite::begin: the workspace, the discovery (order, first_child, the levels; the pointer checks)
//             and the reached-twice check
//   reduce    bottom-up, one launch per level behind the launches of the levels below it.  A group of a level BELOW
//             cut_level gets val[k] = S, the mip of its eight words: byte sums and the count of the non-zero values packed
//             into two registers and added over the group's 8 lanes by three shuffles each.  A group AT or ABOVE cut_level
//             gets val[k] = its uniform field or kNone: every lane resolves its word to a field (a leaf: its own; an
//             interior word of cut_level: VOXEL_OFFSET + S of its group; another interior word: the child's uniform field
//             when the level may merge), compares it with the group's first lane, and the group's byte of the ballot
//             decides.  The same launch gives every child its fate: the field its parent word is rewritten to, or kKeep,
//             and number[child] = kept
//   finish    svo_tree_rewrite::finish over the candidates, the groups whose words lie at or above cut_level: the scan of
//             number, the refusals, the emit and, in place only, the copy back.  A kept group's ancestors are kept (a word
//             is rewritten only together with every word below it), so the order is still breadth-first; an interior lane
//             whose child is not kept writes the leaf word of the child's fate: the tree is rewritten on the fly, never
//             in the node buffer.  Out of place the emit writes the caller's buffer and the node buffer is only read
//
// No atomics and no LDS: the order is the contract.  Every error is decided before the emit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_group.h"  // (group_lane: 8 lanes per group)

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // val: no uniform field (a field has 28 bits)
constexpr uint32_t kKeep = SVO_FATE_KEEP;  // fate: the group stays
enum Mode { kModeMip, kModeCut, kModeMerge };  // a level below cut_level, cut_level itself, any other

// The level order[off, off + n), behind the launches of the levels below it.  may_merge: SVO_SIMPLIFY_MERGE is set and
// the level is not below min_level.
__global__ __launch_bounds__(kThreads) void simplify_reduce_kernel(const uint32_t *words, const uint32_t *order, uint32_t off, uint32_t n,
                                                                   const uint32_t *first_child, int mode, bool may_merge, bool merge,
                                                                   uint32_t *val, uint32_t *fate, uint32_t *number) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const bool valid = k < n;
    const GroupLane g = group_lane(words, order + off, k, c, valid);
    const uint32_t child = g.interior ? first_child[off + k] + g.below : 0u;
    const uint32_t below = g.interior ? val[child] : 0u;
    if (mode == kModeMip) {
        const uint32_t s = g.interior ? below : g.pointer - SVO_VOXEL_OFFSET;
        // sums of at most 8 * 255 and a count of at most 8: 16 bits each
        uint32_t rg = s ? (s & 0xFFu) | (s >> 8 & 0xFFu) << 16 : 0u, bn = s ? (s >> 16 & 0xFFu) | 1u << 16 : 0u;
        for (uint32_t d = 1; d < 8; d <<= 1) {
            rg += __shfl_xor(rg, d);
            bn += __shfl_xor(bn, d);
        }
        if (valid && c == 0) {
            const uint32_t m = bn >> 16;
            uint32_t mip = 0;
            if (m) mip = max(1u, (rg & 0xFFFFu) / m) | max(1u, (rg >> 16) / m) << 8 | max(1u, (bn & 0xFFFFu) / m) << 16;
            val[off + k] = mip;
        }
        return;
    }
    // the field this lane's word is rewritten to, or kKeep; a leaf's field is its own
    uint32_t to = kKeep;
    if (g.interior) {
        if (mode == kModeCut) to = SVO_VOXEL_OFFSET + below;
        else if (may_merge && below != kNone) to = below;
        fate[child] = to;
        number[child] = to == kKeep ? 1u : 0u;
    }
    const uint32_t field = g.interior ? to : g.pointer;  // (kKeep == kNone: an interior word that stays is not uniform)
    const uint32_t first = __shfl(field, __lane_id() & ~7u);
    const uint32_t same = uint32_t(__ballot(field == first && field != kNone) >> (__lane_id() & ~7u)) & 0xFFu;
    if (valid && c == 0) {
        val[off + k] = merge && same == 0xFFu ? first : kNone;
        if (off + k == 0) fate[0] = kKeep, number[0] = 1u;  // the root group has no parent word
    }
}

}  // namespace

// Per-context workspace of the simplification (svo_ctx::simplify): the rewrite's (svo_ctx.h: five u32 per group and, for
// in-place calls, the image) and a sixth u32 per group.
struct svo_simplify_state : svo_tree_rewrite {
    svo_dev<uint32_t> val;  // the mip or the uniform field of a group
};

extern "C" {

int svo_nodes_simplify(svo_ctx *ctx, const svo_simplify_params *p, uint32_t *out_dev, uint32_t *perm_out_dev, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    int rc = svo_check_flags(ctx, p->flags, SVO_SIMPLIFY_MERGE | SVO_SIMPLIFY_CUT);
    if (rc) return rc;
    const bool merge = p->flags & SVO_SIMPLIFY_MERGE, cut = p->flags & SVO_SIMPLIFY_CUT;
    if (!p->flags) return svo_fail(ctx, SVO_ERR_ARG, "flags 0: nothing to simplify (svo_nodes_compact lays a tree out anew)");
    if (cut ? p->cut_level < 1 || p->cut_level > 31 : p->cut_level != 0)
        return svo_fail(ctx, SVO_ERR_ARG, "cut_level must be 1..31 with SVO_SIMPLIFY_CUT and 0 without (got " + std::to_string(p->cut_level) + ")");
    if (!merge && p->min_level) return svo_fail(ctx, SVO_ERR_ARG, "min_level must be 0 without SVO_SIMPLIFY_MERGE (got " + std::to_string(p->min_level) + ")");
    if (p->reserved) return svo_fail(ctx, SVO_ERR_ARG, "reserved must be 0");
    if ((rc = svo_check_store(ctx))) return rc;
    if (!out_dev && ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: its positions and hole stack index the layout "
                                            "that an in-place simplification replaces");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->simplify))) return rc;
    svo_simplify_state *s = ctx->simplify.get();
    if ((rc = s->begin(ctx, p->n_words, !out_dev)) || (rc = svo_grow(ctx, s->walk.cap, &s->val))) return rc;
    const std::vector<uint32_t> &level_off = s->walk.level_off;
    const uint32_t n_levels = (uint32_t)level_off.size() - 1;

    // reduce: the words of order[level_off[l], level_off[l + 1]) are of level l + 1
    for (uint32_t l = n_levels; l-- > 0;) {
        const uint32_t level = l + 1, m = level_off[l + 1] - level_off[l];
        const int mode = cut && level > p->cut_level ? kModeMip : cut && level == p->cut_level ? kModeCut : kModeMerge;
        simplify_reduce_kernel<<<svo_div_up(8ull * m, kThreads), kThreads, 0, ctx->stream>>>(
            ctx->nodes, s->walk.order, level_off[l], m, s->walk.first_child, mode, merge && level >= p->min_level, merge, s->val, s->fate,
            s->number());
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, SVO_REWRITE_MIDDLE));

    // the candidates of the emit: the groups below cut_level are cut off
    const uint32_t total = level_off[cut ? std::min(n_levels, p->cut_level) : n_levels];
    return s->finish(ctx, total, out_dev, p->out_cap, perm_out_dev, p->n_words, n_words_out);
}

int svo_simplify_timing(svo_ctx *ctx, float ms_out[SVO_SIMPLIFY_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->simplify) return svo_fail(ctx, SVO_ERR_STATE, "no tree simplified on this context yet");
    return ctx->simplify->timer.read(ctx, ms_out);
}

}  // extern "C"

// svo_compact.hip -- the tree in the node buffer compacted in place: unreachable groups dropped, with
// SVO_COMPACT_PRUNE_EMPTY also the groups that hold nothing, the rest in the canonical breadth-first order of the
// builder (svo_nodes_relayout(words, n, 32, ...) of the host).  Scans instead of atomics, so the words do not depend on
// the run.  Every kernel gives 8 lanes to a group, one word per lane: a wave64 handles 8 groups, a group is one 32-byte
// read, and its interior mask is its byte of the wave's ballot.
//
//   discover  top-down, one launch set per level: the frontier (old group starts, order[off .. off + F)) counts its
//             interior words per group, an exclusive scan of the counts (svo_scan_u32)       gives every group the place
//             of its first child in the next frontier, and the scatter appends the children behind the frontier at
//             scan + (interior lanes below), which keeps the order of the parents.  first_child[k] = the index in `order`
//             of group k's first interior child.  A pointer that is no multiple of 8 or leaves the words sets a status
//             word; the next frontier's size comes back with the status, once per level
//   check     new_of[order[k] / 8] = k by plain stores, then a launch of its own tests new_of[order[k] / 8] == k: of two
//             groups k that share an old group one store wins and the other k sees it, whichever it is
//   prune     bottom-up, one launch per level: a group is live when any word is a non-empty leaf or an interior word
//             whose child is live, and the root is.  number[k] = live, fate[k] = keep or, of a dead group, the empty
//             field that its parent's word becomes.  Without the flag the two arrays are filled: every group is live
//   emit      one exclusive scan of number over the candidates gives every kept group its new number (level-major, and a
//             kept group's ancestors are kept: still breadth-first).  A kept group's lane writes its word, an interior
//             lane the pointer to its child's new place or the leaf of the child's fate.  In place the groups are
//             written into a workspace image, not into the node buffer they are read from; the optional perm is written here
//   copy back in place: one device-to-device copy of the image and one fill of the freed tail with the empty word
//
// Discover and check are svo_tree_discover, for the voxel listing too (svo_list.hip).  Everything but the prune is
// svo_tree_rewrite (svo_ctx.h), the frame that the simplification (svo_simplify.hip) runs around its reduce: begin() up to
// the check, finish() from the scan on.  Every error is decided before the emit, so it leaves the node buffer, the
// caller's buffer and the perm as they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_group.h"  // (group_lane: 8 lanes per group; kMaxWords)
#include "svo_scan.h"   // (svo_scan_u32)

namespace {

constexpr uint32_t kMaxLevels = 31;               // as svo_nodes_relayout and svo_nodes_max_depth
// the words read back: the discovery's (svo_ctx.h), then the rewrite's own
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStKept = SVO_WALK_STATUS, kStWords };

// The frontier order[0, n) (the caller passes order + off): count[k] = interior words of group k; the pointers are checked.
__global__ __launch_bounds__(kThreads) void compact_count_kernel(const uint32_t *words, uint32_t n_words, const uint32_t *order,
                                                                 uint32_t n, uint32_t *count, uint32_t *status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const GroupLane g = group_lane(words, order, k, c, k < n);
    if (g.interior) {  // (every writer stores the same value)
        if (g.pointer & 7u) status[kStAlign] = 1u;
        else if (g.pointer + 8u > n_words) status[kStRange] = 1u;
    }
    if (k < n && c == 0) count[k] = __popc(g.mask);
}

// The frontier order[off, off + n) and the exclusive scan of its counts: the children go behind it, in the parents' order.
__global__ __launch_bounds__(kThreads) void compact_scatter_kernel(const uint32_t *words, uint32_t *order, uint32_t off, uint32_t n,
                                                                   const uint32_t *scan, uint32_t *first_child, uint32_t cap,
                                                                   uint32_t *status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const GroupLane g = group_lane(words, order + off, k, c, k < n);
    if (k >= n) return;
    const uint32_t first = off + n + scan[k];
    if (g.interior && first + g.below < cap) order[first + g.below] = g.pointer;  // (more than cap: a group reached twice, refused on the host)
    if (c == 0) {
        first_child[off + k] = first;
        if (k == n - 1) status[kStNext] = scan[k] + __popc(g.mask);
    }
}

__global__ __launch_bounds__(kThreads) void compact_mark_kernel(const uint32_t *order, uint32_t n, uint32_t *new_of) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n) new_of[order[k] >> 3] = k;
}

__global__ __launch_bounds__(kThreads) void compact_check_kernel(const uint32_t *order, uint32_t n, const uint32_t *new_of,
                                                                 uint32_t *status) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n && new_of[order[k] >> 3] != k) status[kStDup] = 1u;
}

// The level order[off, off + n), behind the launches of the levels below it: number[k] = the group is live, and its fate.
__global__ __launch_bounds__(kThreads) void compact_live_kernel(const uint32_t *words, const uint32_t *order, uint32_t off, uint32_t n,
                                                                const uint32_t *first_child, uint32_t *number, uint32_t *fate) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const bool valid = k < n;
    const GroupLane g = group_lane(words, order + off, k, c, valid);
    const bool keeps = valid && (g.interior ? number[first_child[off + k] + g.below] != 0u : g.pointer != SVO_VOXEL_OFFSET);
    const uint32_t any = uint32_t(__ballot(keeps) >> (__lane_id() & ~7u)) & 0xFFu;
    if (valid && c == 0) {
        const bool live = any || off + k == 0;  // the root group has no parent word
        number[off + k] = live ? 1u : 0u;
        fate[off + k] = live ? SVO_FATE_KEEP : SVO_VOXEL_OFFSET;  // (the parent's word becomes the empty word)
    }
}

// behind the scan of number[0, n): how many groups stay
__global__ void rewrite_total_kernel(const uint32_t *number, const uint32_t *fate, uint32_t n, uint32_t *status) {
    status[kStKept] = number[n - 1] + (fate[n - 1] == SVO_FATE_KEEP ? 1u : 0u);
}

// The candidates order[0, n): a kept group's words, an interior word as the pointer to its child's new place or as the
// leaf of the child's fate.
__global__ __launch_bounds__(kThreads) void rewrite_emit_kernel(const uint32_t *words, const uint32_t *order, uint32_t n,
                                                                const uint32_t *first_child, const uint32_t *fate,
                                                                const uint32_t *number, uint32_t n_out, uint32_t *image, uint32_t *perm) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const bool valid = k < n;
    const GroupLane g = group_lane(words, order, k, c, valid);
    if (!valid || fate[k] != SVO_FATE_KEEP) return;
    uint32_t out = g.word;
    if (g.interior) {
        const uint32_t child = first_child[k] + g.below, to = fate[child];  // (a child behind the candidates has a fate too)
        out = to == SVO_FATE_KEEP ? ((8u * number[child]) << 4 | (g.word & 15u)) : to << 4;
    }
    const uint32_t at = 8u * number[k] + c;
    if (at < n_out) {  // (always: n_out is the scan's total)
        image[at] = out;
        if (perm) perm[at] = order[k] + c;
    }
}

int malformed(svo_ctx *ctx, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, "malformed tree: " + why); }

}  // namespace

// Per-context workspace of the compaction (svo_ctx::compact): the rewrite's (svo_ctx.h), the image and five u32 per group.
struct svo_compact_state : svo_tree_rewrite {};

// The discovery and the check of the tree in the first n_words_in words of the node buffer, on the ctx stream into the
// walk's workspace (svo_ctx.h), which the caller has grown.  Blocks once per level.
int svo_tree_discover(svo_ctx *ctx, uint64_t n_words_in, svo_tree_walk *w, hipEvent_t discovered) {
    // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
    const uint32_t n_words = (uint32_t)std::min<uint64_t>(n_words_in, kMaxWords), cap = n_words / 8;
    w->n_words = n_words, w->cap = cap;
    const uint32_t *st = w->status.host();
    int rc;
    HIP_TRY(ctx, hipMemsetAsync(w->order, 0, sizeof(uint32_t), ctx->stream));  // level 1: group 0

    // discover
    std::vector<uint32_t> &level_off = w->level_off;
    level_off.clear();
    uint32_t off = 0, n = 1;
    for (uint32_t level = 1;; level++) {
        level_off.push_back(off);
        const uint32_t grid = svo_div_up(8ull * n, kThreads);
        compact_count_kernel<<<grid, kThreads, 0, ctx->stream>>>(ctx->nodes, n_words, w->order + off, n, w->scan, w->status.dev);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = svo_scan_u32(ctx, w->scan, n))) return rc;
        compact_scatter_kernel<<<grid, kThreads, 0, ctx->stream>>>(ctx->nodes, w->order, off, n, w->scan, w->first_child, cap, w->status.dev);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = w->status.read(ctx))) return rc;
        if (st[kStAlign]) return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " is not a multiple of 8");
        if (st[kStRange])
            return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " leaves the first n_words = " +
                                      std::to_string(n_words_in) + " words");
        const uint32_t next = st[kStNext];
        if (uint64_t(off) + n + next > cap)
            return malformed(ctx, "a group is reached twice (level " + std::to_string(level + 1) + " brings the groups reached to " +
                                      std::to_string(uint64_t(off) + n + next) + ", more than n_words / 8)");
        off += n;
        if (!next) break;
        if (level == kMaxLevels) return malformed(ctx, "the tree is deeper than " + std::to_string(kMaxLevels) + " levels");
        n = next;
    }
    const uint32_t total = off;
    level_off.push_back(total);
    if (discovered) HIP_TRY(ctx, hipEventRecord(discovered, ctx->stream));

    // check (the verdict is in status[SVO_WALK_DUP] at the caller's next read-back)
    const uint32_t group_grid = svo_div_up(total, kThreads);
    compact_mark_kernel<<<group_grid, kThreads, 0, ctx->stream>>>(w->order, total, w->new_of);
    compact_check_kernel<<<group_grid, kThreads, 0, ctx->stream>>>(w->order, total, w->new_of, w->status.dev);
    HIP_TRY(ctx, hipGetLastError());
    return SVO_OK;
}

int svo_tree_rewrite::create(svo_ctx *ctx) {
    HIP_TRY(ctx, timer.create());
    return walk.create(ctx, kStWords);
}

int svo_tree_rewrite::begin(svo_ctx *ctx, uint64_t n_words_in, bool in_place) {
    t0 = svo_now_ms();
    const size_t n_words = (size_t)std::min<uint64_t>(n_words_in, kMaxWords);
    int rc;
    if (in_place && (rc = svo_grow(ctx, n_words, &image))) return rc;
    if ((rc = walk.grow(ctx, n_words / 8)) || (rc = svo_grow(ctx, n_words / 8, &fate))) return rc;
    if ((rc = timer.begin(ctx))) return rc;
    // the passes read the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, timer.mark(ctx, SVO_REWRITE_START));
    HIP_TRY(ctx, walk.status.zero(ctx));
    if ((rc = svo_tree_discover(ctx, n_words_in, &walk, timer.ev[SVO_REWRITE_DISCOVER]))) return rc;
    HIP_TRY(ctx, timer.mark(ctx, SVO_REWRITE_CHECK));
    return SVO_OK;
}

int svo_tree_rewrite::finish(svo_ctx *ctx, uint32_t total, uint32_t *out_dev, uint64_t out_cap, uint32_t *perm_out_dev,
                             uint64_t n_words_in, uint64_t *n_words_out) {
    const uint32_t *st = walk.status.host();
    int rc;
    if ((rc = svo_scan_u32(ctx, number(), total))) return rc;
    rewrite_total_kernel<<<1, 1, 0, ctx->stream>>>(number(), fate, total, walk.status.dev);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = walk.status.read(ctx))) return rc;
    if (st[kStDup]) return malformed(ctx, "a group is reached twice");
    const uint32_t n_out = 8u * st[kStKept];
    if (!n_out || n_out > walk.n_words) return svo_fail(ctx, SVO_ERR_HIP, "the kept groups' scan is out of range");  // (never: the root stays)
    if (out_dev && n_out > out_cap)
        return svo_fail(ctx, SVO_ERR_CAP, "the simplified tree has " + std::to_string(n_out) + " words, more than out_cap = " +
                                              std::to_string(out_cap));
    rewrite_emit_kernel<<<svo_div_up(8ull * total, kThreads), kThreads, 0, ctx->stream>>>(
        ctx->nodes, walk.order, total, walk.first_child, fate, number(), n_out, out_dev ? out_dev : image.get(), perm_out_dev);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, timer.mark(ctx, SVO_REWRITE_EMIT));

    if (!out_dev) {
        // copy back: behind every earlier write to the store (another context may have written while this one waited)
        if ((rc = svo_store_order_after_write(ctx))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->nodes, image, size_t(n_out) * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        if (n_words_in > n_out)
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(ctx->nodes + n_out), (int)kEmptyWord, n_words_in - n_out, ctx->stream));
    }
    HIP_TRY(ctx, timer.mark(ctx, SVO_REWRITE_END));
    if (!out_dev && (rc = svo_store_note_write(ctx))) return rc;
    *n_words_out = n_out;
    timer.finish(t0);
    return SVO_OK;
}

extern "C" {

int svo_nodes_compact(svo_ctx *ctx, const svo_compact_params *p, uint32_t *perm_out_dev, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    int rc = svo_check_flags(ctx, p->flags, SVO_COMPACT_PRUNE_EMPTY);
    if (rc || (rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: its positions and hole stack index the layout "
                                            "that a compaction replaces");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->compact))) return rc;
    svo_compact_state *s = ctx->compact.get();
    if ((rc = s->begin(ctx, p->n_words, true))) return rc;
    const std::vector<uint32_t> &level_off = s->walk.level_off;
    const uint32_t n_levels = (uint32_t)level_off.size() - 1, total = level_off[n_levels];

    // prune
    if (p->flags & SVO_COMPACT_PRUNE_EMPTY) {
        for (uint32_t l = n_levels; l-- > 0;) {
            const uint32_t m = level_off[l + 1] - level_off[l];
            compact_live_kernel<<<svo_div_up(8ull * m, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, s->walk.order, level_off[l], m,
                                                                                             s->walk.first_child, s->number(), s->fate);
        }
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)s->number(), 1, total, ctx->stream));
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)s->fate.get(), (int)SVO_FATE_KEEP, total, ctx->stream));
    }
    HIP_TRY(ctx, s->timer.mark(ctx, SVO_REWRITE_MIDDLE));
    return s->finish(ctx, total, nullptr, 0, perm_out_dev, p->n_words, n_words_out);
}

int svo_compact_timing(svo_ctx *ctx, float ms_out[SVO_COMPACT_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->compact) return svo_fail(ctx, SVO_ERR_STATE, "no tree compacted on this context yet");
    return ctx->compact->timer.read(ctx, ms_out);
}

}  // extern "C"

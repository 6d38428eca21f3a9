// svo_edit.hip -- voxels inserted into and removed from a tree that is already in the node buffer: the
// device form of sequential put(p, leaf, depth) over the distinct cells of a voxel list in ascending Morton-key order.
// The edit touches O(voxels * depth) words and, like the builder, uses scans instead of atomics, so the words do not
// depend on the run or on the order of distinct input voxels.
//
//   leaves   the builder's list front end (svo_build_list_leaves): keys, stable sort, the last voxel of every cell
//   plan     one lane per distinct voxel k, reading only: the walk of the words as they are from group 0 gives l0, the
//            level of the first leaf on the voxel's path, and that leaf's index; an interior word at `depth` refuses
//            the call.  c = the leading levels key k shares with key k - 1.  l = max(l0, c + 1) (l0 for k = 0) is the
//            level of the leaf the host finds when it gets to voxel k: every earlier voxel split the path down to the
//            prefix it shares with k, and in Morton order no earlier voxel shares more with k than its predecessor.
//            Voxel k creates depth - l groups
//   scan     exclusive scan of the group counts (svo_scan_u32): start_k.  One block then finds the first voxel
//            that cannot be taken and the total; both come back with the counts in one small copy, and the cap is
//            checked on the host before anything is written
//   fill     the new groups [n_words, n_words + 8 * total) become empty words
//   link     lane k writes its path: the pointer to group n_words + 8 * (start_k + j - l) into its node of level j,
//            j = l .. depth - 1, and its leaf into the node of level `depth`.  The node of level l is the original leaf
//            when l == l0; otherwise it is a slot of the group below the shared prefix of c levels, which the head of
//            the run of voxels sharing that prefix made as its group c - l_head (found by bisection on the keys).  No two
//            lanes write the same word; the fill is a launch of its own before them
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_ctx.h"
#include "svo_morton.h"  // (the key's convention; the refused voxel's cell)
#include "svo_scan.h"    // (svo_scan_u32, block_exclusive_scan, input_count; svo_group.h: kEmptyWord, kMaxWords)

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMalformed = 1u << 31;  // in a block's first untakeable voxel: its walk left the tree
enum Status { kStCount, kStRange, kStGroups, kStBad, kStIndex, kStKeyLo, kStKeyHi, kStWords };  // the words read back
enum Bad { kBadNone = 0, kBadRefused = 1, kBadMalformed = 2 };

__device__ inline uint32_t child_at(uint64_t key, uint32_t level, uint32_t depth) { return uint32_t(key >> (3 * (depth - level))) & 7u; }

// lvl[k] = l | l0 << 8, start[k] = depth - l (0 behind the m distinct voxels, so that one scan covers the host's bound),
// at[k] = the index of the first leaf on the path; bad[block] = the block's first voxel that cannot be taken, or kNone.
__global__ __launch_bounds__(kThreads) void edit_plan_kernel(const uint32_t *words, uint32_t n_words, const uint64_t *keys,
                                                             const uint32_t *m_dev, uint32_t m_max, uint32_t depth, uint32_t *lvl,
                                                             uint32_t *start, uint32_t *at, uint32_t *bad) {
    __shared__ uint32_t wave_first[kThreads / 64];
    const uint32_t m = input_count(m_dev, m_max);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    uint32_t why = kBadNone, l0 = 0, l = depth, leaf = 0;
    if (k < m) {
        const uint64_t key = keys[k];
        uint32_t base = 0;
        for (uint32_t level = 1; level <= depth; level++) {
            const uint32_t a = base + child_at(key, level, depth);
            if (a >= n_words) {
                why = kBadMalformed;
                break;
            }
            const uint32_t pointer = words[a] >> 4;
            if (pointer >= SVO_VOXEL_OFFSET) {
                l0 = level;
                leaf = a;
                break;
            }
            if (level == depth) why = kBadRefused;
            base = pointer;
        }
        if (why == kBadNone) {
            l = l0;
            if (k) {  // (distinct keys: the xor is not 0)
                const uint32_t c = (uint32_t(__clzll((long long)(key ^ keys[k - 1]))) - (64u - 3u * depth)) / 3u;
                l = max(l0, c + 1);
            }
        }
    }
    if (k < m_max) {
        lvl[k] = l | l0 << 8;
        start[k] = depth - l;
        at[k] = leaf;
    }
    const uint64_t any = __ballot(why != kBadNone);
    const uint32_t first = any ? uint32_t(__ffsll((long long)any)) - 1u : 0u;
    const uint32_t first_why = __shfl(why, first);
    if ((threadIdx.x & 63u) == 0)
        wave_first[threadIdx.x / 64] = any ? ((k + first) | (first_why == kBadMalformed ? kMalformed : 0u)) : kNone;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t b = kNone;
        for (uint32_t w = kThreads / 64; w-- > 0;)
            if (wave_first[w] != kNone) b = wave_first[w];
        bad[blockIdx.x] = b;
    }
}

// One block, after the scan: the counts, the total of new groups and the first voxel (in key order) that cannot be taken.
__global__ __launch_bounds__(kTopThreads) void edit_status_kernel(const uint32_t *bad, uint32_t n_blocks, const uint32_t *m_dev,
                                                                  uint32_t m_max, const uint32_t *range_err, uint32_t depth,
                                                                  const uint32_t *lvl, const uint32_t *start, const uint64_t *keys,
                                                                  const uint32_t *index, uint32_t *status) {
    const uint32_t m = input_count(m_dev, m_max);
    const uint32_t per = (n_blocks + kTopThreads - 1) / kTopThreads;
    const uint32_t lo = min(threadIdx.x * per, n_blocks), hi = min(lo + per, n_blocks);
    uint32_t mine = kNone;
    for (uint32_t b = hi; b-- > lo;)
        if (bad[b] != kNone) mine = bad[b];
    uint32_t found;
    const uint32_t before = block_exclusive_scan<kTopThreads>(mine != kNone, &found);
    if (mine != kNone && before == 0) {
        const uint32_t k = mine & ~kMalformed;
        status[kStBad] = mine & kMalformed ? kBadMalformed : kBadRefused;
        status[kStIndex] = index[k];
        status[kStKeyLo] = uint32_t(keys[k]);
        status[kStKeyHi] = uint32_t(keys[k] >> 32);
    }
    if (threadIdx.x == 0) {
        status[kStCount] = m;
        status[kStRange] = *range_err;
        status[kStGroups] = m ? start[m - 1] + depth - (lvl[m - 1] & 0xFFu) : 0u;
        if (!found) status[kStBad] = kBadNone;
    }
}

__global__ __launch_bounds__(kThreads) void edit_link_kernel(uint32_t *words, uint32_t n_words, uint32_t new_words, const uint64_t *keys,
                                                             const uint32_t *colours, uint32_t m, uint32_t depth, const uint32_t *lvl,
                                                             const uint32_t *start, const uint32_t *at) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= m) return;
    const uint64_t key = keys[k];
    const uint32_t l = lvl[k] & 0xFFu, l0 = lvl[k] >> 8, s = start[k];
    uint32_t a = at[k];
    if (l != l0) {  // l = c + 1 > l0: a slot of the group that the head of the run sharing c levels made below them
        const uint32_t c = l - 1, shift = 3 * (depth - c);
        const uint64_t prefix = key >> shift;
        uint32_t lo = 0, hi = k;  // the first i with keys[i] >> shift == prefix (k itself if no earlier one)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((keys[mid] >> shift) < prefix) lo = mid + 1;
            else hi = mid;
        }
        a = n_words + 8u * (start[lo] + c - (lvl[lo] & 0xFFu)) + child_at(key, l, depth);
    }
    for (uint32_t j = l; j < depth; j++) {
        const uint32_t group = n_words + 8u * (s + j - l);
        if (a < new_words) words[a] = group << 4;  // (always: the plan and the scan come from the same words)
        a = group + child_at(key, j + 1, depth);
    }
    if (a < new_words) words[a] = (SVO_VOXEL_OFFSET + colours[k]) << 4;
}

enum Ev { kEvPlan, kEvRead, kEvFill, kEvEnd, kEvs };

}  // namespace

// Per-context workspace of the edit (svo_ctx::edit).  The per-voxel arrays live in the builder's workspace, in the sort
// buffers its front end no longer needs (svo_build_leaves::spare32 / spare64); what is the edit's own is the status words
// and the events.  The first three spans of its times run between the builder's events, which the front end hands out.
struct svo_edit_state {
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_EDIT_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

extern "C" {

int svo_nodes_edit(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_edit_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    int rc = svo_build_check_list(ctx, p ? &p->depth : nullptr, xyz, n);
    if (rc) return rc;
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->edit))) return rc;
    svo_edit_state *s = ctx->edit.get();
    if (!n) {  // nothing to edit
        s->timer.none();
        *n_words_out = p->n_words;
        return SVO_OK;
    }
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;  // (before the front end records the builder's events again)
    const uint32_t depth = p->depth, n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), bound = (uint32_t)n;
    svo_build_leaves lv{};
    if ((rc = svo_build_list_leaves(ctx, xyz, colours, n, depth, p->default_colour, &lv))) return rc;
    uint32_t *lvl = lv.spare32, *start = (uint32_t *)lv.spare64[0], *at = start + lv.items, *bad = (uint32_t *)lv.spare64[1];
    const uint32_t n_blocks = svo_div_up(bound, kThreads);

    // the plan reads the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    edit_plan_kernel<<<n_blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, n_words, lv.keys, lv.count, bound, depth, lvl, start, at, bad);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = svo_scan_u32(ctx, start, bound))) return rc;
    edit_status_kernel<<<1, kTopThreads, 0, ctx->stream>>>(bad, n_blocks, lv.count, bound, lv.range_err, depth, lvl, start, lv.keys,
                                                          lv.index, s->status.dev);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvPlan));
    HIP_TRY(ctx, s->status.copy(ctx));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvRead));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    const uint32_t *st = s->status.host();
    if (st[kStRange])
        return svo_fail(ctx, SVO_ERR_ARG, "a voxel coordinate is outside [0, 2^depth) (depth " + std::to_string(depth) + ")");
    if (st[kStBad]) {
        uint32_t x, y, z;
        morton_decode(uint64_t(st[kStKeyHi]) << 32 | st[kStKeyLo], depth, x, y, z);
        const std::string who = "voxel " + std::to_string(st[kStIndex]) + " (cell " + std::to_string(x) + ", " + std::to_string(y) + ", " +
                                std::to_string(z) + ")";
        if (st[kStBad] == kBadMalformed)
            return svo_fail(ctx, SVO_ERR_STATE, who + ": its path leaves the first n_words = " + std::to_string(n_words) + " words of the tree");
        return svo_fail(ctx, SVO_ERR_STATE, who + " is an interior node at depth " + std::to_string(depth) +
                                                ": the tree is finer there than the edit, which replaces no subtree");
    }
    uint64_t limit = std::min<uint64_t>(ctx->capacity, kMaxWords);
    if (p->max_words) limit = std::min<uint64_t>(limit, p->max_words);
    // every distinct voxel ends in a word of its own, so more of them than words can be cannot fit (and up to there the u32
    // scan is exact: 2^27 * 20 < 2^32)
    const uint64_t new_words = st[kStCount] > kMaxWords ? ~0ull : p->n_words + 8ull * st[kStGroups];
    if (new_words > limit)
        return svo_fail(ctx, SVO_ERR_CAP, (st[kStCount] > kMaxWords ? "the edited tree needs more than 2^27 words"
                                                                     : "the edited tree needs " + std::to_string(new_words) + " words") +
                                              ", over the limit of " + std::to_string(limit) + " (max_words, the node buffer's capacity, 2^27)");

    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvFill));
    if (new_words > p->n_words)
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(ctx->nodes + p->n_words), (int)kEmptyWord, new_words - p->n_words, ctx->stream));
    edit_link_kernel<<<svo_div_up(st[kStCount], kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, n_words, (uint32_t)new_words, lv.keys,
                                                                                      lv.colours, st[kStCount], depth, lvl, start, at);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEnd));
    if ((rc = svo_store_note_write(ctx))) return rc;
    *n_words_out = new_words;
    const svo_events<kEvs> &ev = s->timer.ev;
    const hipEvent_t span[SVO_EDIT_TIMES - 1][2] = {
        {lv.ev_start, lv.ev_keys}, {lv.ev_keys, lv.ev_sort}, {lv.ev_sort, ev[kEvPlan]}, {ev[kEvPlan], ev[kEvRead]}, {ev[kEvFill], ev[kEvEnd]}};
    memcpy(s->timer.span, span, sizeof span);
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_edit_timing(svo_ctx *ctx, float ms_out[SVO_EDIT_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->edit) return svo_fail(ctx, SVO_ERR_STATE, "no tree edited on this context yet");
    return ctx->edit->timer.read(ctx, ms_out);
}

}  // extern "C"

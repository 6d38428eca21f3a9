// svo_combine.hip -- two trees combined: the tree in the node buffer, the scene, edited in place by a second
// tree, the source, that is only read: pasted over it, filled under it, painted, carved, masked or put in its place, whole
// or into one cell of a coarser level.  include/svo_hip.h has the rule for one word; this file applies it level by level in
// svo_region.hip's frame, with a tree where that file has shapes.  Scans instead of atomics: the words do not depend on the
// run.
//
//   frontier  the words of a level where both trees have something to say, as groups of eight.  The scene's side of a
//             group is svo_region.hip's: the group's first word (in the buffer, or in a group that a split will make: a
//             *virtual* group, whose eight words are one leaf word kept in the record) and the cell of its parent.  The
//             source's side is one word, read like a word of a tree: an interior field is the source group whose eight
//             words pair with the scene's by child index, a leaf field is a constant carried down that all eight pair
//             with, and kSrcPath in the counter's bits says that the group lies above the placement: one child leads on
//             towards the cell `at`, the other seven lie outside the source.  Level 1 is the root group
//   plan      per level, reading only, one lane per frontier word: the eight lanes of a group read the scene's group and
//             the source's as one 32-byte line each.  The lane decides by a table over the op and whether either value is
//             empty, flags its word opened or split and puts what it would write into the write list, which has one entry
//             per frontier word of every level
//   scan      two in-place scans (svo_scan_u32) of the flags, then the next level's records, as in svo_region.hip; a
//             source pointer that is followed is checked here as a scene pointer is
//   check     every scene group reached through a pointer marks itself in new_of; a mark found or lost is a group reached
//             twice.  A source group may be reached as often as it likes: it is only read
//   status    the first refused word of level `depth` in frontier order (a minimum over the blocks' minima), read back
//   commit    a fill launch writes the eight leaf words of every new group, then one launch writes the list.  Neither reads
//             the source: a graft's words are in the fill values and the list, so check and commit are the region's own
//             kernels (svo_frontier.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_combine_rules.h"  // (combine_value, whole_subtree, whole_constant, leaf_stays)
#include "svo_ctx.h"
#include "svo_frontier.h"  // (kNone, leaf_word, region_mark_kernel, region_check_kernel, region_fill_kernel, region_write_kernel, grow_list)
#include "svo_scan.h"  // (svo_scan_u32, block_min, min_of_blocks_kernel; svo_group.h: kThreads, kEmptyWord, kMaxWords)

namespace {

constexpr uint32_t kCellBits = 21, kCellMask = (1u << kCellBits) - 1u;  // a record's cell: x << 42 | y << 21 | z
constexpr uint32_t kSrcPath = 8u;  // a group's source record: above the placement (no source word has it: the records' low four bits are 0)
enum Src : uint32_t { kOut, kLeaf, kNode };  // what the source has for a frontier word's cube
// a word's flags.  kOpen: eight children in the next frontier; kSplit: ... of a new group; at level `depth`, where neither
// is allowed, which tree is finer under the refused word
enum Code : uint32_t { kOpen = 1u, kSplit = 2u, kSceneFiner = 4u, kSourceFiner = 8u };
// the words read back: the discovery's names for the first four (svo_ctx.h), then this pass's own
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStSplits, kStBad, kStSrcAlign, kStSrcRange, kStWords };

// (the rule's tables over the op and whether either value is empty: svo_combine_rules.h, shared with svo_place.hip)

// The call's constants, by value to the kernels.
struct Placement {
    uint32_t op, depth, at_level, at[3];
};

// What the lane of frontier word i knows of it: where the scene's word is, the word as it stands and its cell on its level;
// what the source has for the same cube: nothing (kOut), the value b (kLeaf), or a subtree (kNode), whose children's
// record is `next`.
struct Pair {
    uint32_t at, word, x, y, z, kind, b, next;
};
__device__ inline Pair frontier_pair(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, const Placement &pl, uint32_t level,
                                     const uint32_t *__restrict__ gbase, const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt,
                                     const uint32_t *__restrict__ gsrc, uint32_t i) {
    const uint32_t g = i >> 3, c = i & 7u, virt = gvirt[g], rec = gsrc[g];
    const uint64_t key = gkey[g];
    Pair e;
    e.at = gbase[g] + c;
    e.word = virt ? virt : words[e.at];  // (a real group's pointer passed the check: below n_words)
    e.x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2);
    e.y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u);
    e.z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
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

// The rule for the n frontier words of `level`.  code[i] = the word's flags, also as the two scans' inputs; list_at[i] =
// the word's address when something is written there (kNone: nothing), list_word[i] = what (a split's pointer comes from
// combine_emit_kernel), list_fill[i] = the leaf word a split's new group is filled with; bad[block] = the block's first
// word, in frontier order, that would be opened or split at level == depth.
__global__ __launch_bounds__(kThreads) void combine_plan_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Placement pl,
                                                                uint32_t level, const uint32_t *__restrict__ gbase,
                                                                const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt,
                                                                const uint32_t *__restrict__ gsrc, uint32_t n, uint32_t *__restrict__ code,
                                                                uint32_t *__restrict__ open_scan, uint32_t *__restrict__ split_scan,
                                                                uint32_t *__restrict__ list_at, uint32_t *__restrict__ list_word,
                                                                uint32_t *__restrict__ list_fill, uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < n) {
        const Pair e = frontier_pair(words, src, pl, level, gbase, gkey, gvirt, gsrc, i);
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        const uint32_t a = leaf ? (e.word >> 4) - SVO_VOXEL_OFFSET : 0u;
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (e.kind == kLeaf) {
            if (leaf) {
                const uint32_t v = combine_value(pl.op, a, e.b);
                if (v != a) at = e.at, out = leaf_word(v);
            } else {
                const uint32_t whole = whole_subtree(pl.op, e.b != 0u);
                if (whole == kConstant) at = e.at, out = leaf_word(whole_constant(pl.op, e.b));  // collapse
                else if (whole == kOpenIt) cd = level == pl.depth ? kSceneFiner : kOpen;
            }
        } else if (e.kind == kNode) {
            if (!leaf) cd = level == pl.depth ? kSceneFiner | kSourceFiner : kOpen;
            else if (!leaf_stays(pl.op, a != 0u)) {
                if (level == pl.depth) cd = kSourceFiner;
                else cd = kOpen | kSplit, at = e.at, fill = e.word & ~15u;
            }
        }
        if (cd & (kSceneFiner | kSourceFiner)) refused = i;
        code[i] = cd;
        open_scan[i] = cd & kOpen;
        split_scan[i] = (cd & kSplit) >> 1;
        list_at[i] = at;
        list_word[i] = out;
        list_fill[i] = fill;
    }
    const uint32_t first = block_min<kThreads>(refused);
    if (threadIdx.x == 0) bad[blockIdx.x] = first;
}

// Behind the two scans: the records of the next frontier's groups, in the order of their parents, the pointers of the
// splits, whose groups start at `first_new` in the order of the scan, and the two totals.  A pointer that is followed, the
// scene's or the source's, is checked as the discovery checks it.
__global__ __launch_bounds__(kThreads) void combine_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Placement pl,
                                                                uint32_t level, const uint32_t *__restrict__ gbase,
                                                                const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt,
                                                                const uint32_t *__restrict__ gsrc, uint32_t n, const uint32_t *__restrict__ code,
                                                                const uint32_t *__restrict__ open_scan, const uint32_t *__restrict__ split_scan,
                                                                uint32_t n_words, uint32_t src_words, uint32_t first_new,
                                                                uint32_t *__restrict__ list_word, uint32_t *__restrict__ next_base,
                                                                uint64_t *__restrict__ next_key, uint32_t *__restrict__ next_virt,
                                                                uint32_t *__restrict__ next_src, uint32_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t cd = code[i], k = open_scan[i];
    if (i == n - 1) {
        status[kStNext] = k + (cd & kOpen);
        status[kStSplits] = split_scan[i] + ((cd & kSplit) >> 1);
    }
    if (!(cd & kOpen) || k >= n) return;  // (k < n always: a word opens one group at the most)
    const Pair e = frontier_pair(words, src, pl, level, gbase, gkey, gvirt, gsrc, i);
    uint32_t base, virt = 0;
    if (cd & kSplit) {
        base = first_new + 8u * split_scan[i];
        virt = e.word & ~15u;
        list_word[i] = base << 4;
    } else {
        base = e.word >> 4;
        if (base & 7u) status[kStAlign] = 1u;  // (every writer stores the same value)
        else if (uint64_t(base) + 8u > n_words) status[kStRange] = 1u;
    }
    uint32_t rec = e.next;
    if (e.kind == kLeaf) rec = leaf_word(e.b);  // the constant, carried down
    else if (rec != kSrcPath) {
        if ((rec >> 4) & 7u) status[kStSrcAlign] = 1u;
        else if (uint64_t(rec >> 4) + 8u > src_words) status[kStSrcRange] = 1u;
    }
    next_base[k] = base;
    next_virt[k] = virt;
    next_src[k] = rec;
    next_key[k] = uint64_t(e.x) << (2 * kCellBits) | uint64_t(e.y) << kCellBits | e.z;
}

// (the scene's groups mark themselves and are checked by svo_frontier.h's region_mark_kernel and region_check_kernel, and
// its region_fill_kernel and region_write_kernel are the commit: the region's kernels, shared)

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// Per-context workspace of the combine (svo_ctx::combine): two sets of frontier records that the levels take turns in, the
// per-word arrays of one level, the write list of all levels, and the marks.
struct svo_combine_state {
    svo_dev<uint32_t> gbase[2], gvirt[2], gsrc[2];
    svo_dev<uint64_t> gkey[2];
    svo_dev<uint32_t> code, open_scan, split_scan, bad;
    svo_dev<uint32_t> list_at, list_word, list_fill;
    svo_dev<uint32_t> new_of;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_COMBINE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

namespace {

int malformed(svo_ctx *ctx, const char *which, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, std::string("malformed ") + which + ": " + why); }

const char *const kOpNames[] = {"over", "under", "paint", "carve", "keep", "replace"};

}  // namespace

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
    // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
    const uint32_t depth = p->depth, n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), cap = n_words / 8;
    const uint32_t src_words = (uint32_t)p->src_words;
    const Placement pl = {p->op, depth, p->at_level, {p->at[0], p->at[1], p->at[2]}};
    if ((rc = svo_grow(ctx, (size_t)cap, &s->new_of))) return rc;
    const uint32_t *st = s->status.host();

    // the plan reads the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    HIP_TRY(ctx, s->status.zero(ctx));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0xFF, size_t(cap) * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0, sizeof(uint32_t), ctx->stream));  // the root group is group 0 of the frontiers
    if ((rc = svo_grow(ctx, 1, &s->gbase[0], &s->gvirt[0], &s->gsrc[0])) || (rc = svo_grow(ctx, 1, &s->gkey[0]))) return rc;
    // level 1: the scene's root group, real, its parent the cell 0, against the source's root group or the path to `at`
    HIP_TRY(ctx, hipMemsetAsync(s->gbase[0], 0, sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->gvirt[0], 0, sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)s->gsrc[0].get(), p->at_level ? (int)kSrcPath : 0, 1, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->gkey[0], 0, sizeof(uint64_t), ctx->stream));

    // plan: off = the frontier words of the levels above (the list's entries so far), n = this level's
    uint64_t off = 0, groups_seen = 1, splits = 0;
    uint32_t n = 8, last_blocks = 0, last_level = 0;
    int cur = 0;
    for (uint32_t level = 1; level <= depth && n; level++, cur ^= 1) {
        // every frontier word is a word of its own of the combined tree
        if (off + n > kMaxWords + 8ull * cap)
            return svo_fail(ctx, SVO_ERR_CAP, "the combined tree needs more than 2^27 words, over the limit (max_words, the node buffer's capacity, 2^27)");
        const int nx = cur ^ 1;
        const uint32_t blocks = svo_div_up(n, kThreads);
        if ((rc = svo_grow(ctx, (size_t)n, &s->code, &s->open_scan, &s->split_scan)) || (rc = svo_grow(ctx, (size_t)blocks, &s->bad)) ||
            (rc = svo_grow(ctx, (size_t)n, &s->gbase[nx], &s->gvirt[nx], &s->gsrc[nx])) || (rc = svo_grow(ctx, (size_t)n, &s->gkey[nx])) ||
            (rc = grow_list(ctx, off + n, off, &s->list_at, &s->list_word, &s->list_fill)))
            return rc;
        combine_plan_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src_dev, pl, level, s->gbase[cur], s->gkey[cur], s->gvirt[cur],
                                                                 s->gsrc[cur], n, s->code, s->open_scan, s->split_scan, s->list_at + off,
                                                                 s->list_word + off, s->list_fill + off, s->bad);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = svo_scan_u32(ctx, s->open_scan, n)) || (rc = svo_scan_u32(ctx, s->split_scan, n))) return rc;
        combine_emit_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src_dev, pl, level, s->gbase[cur], s->gkey[cur], s->gvirt[cur],
                                                                 s->gsrc[cur], n, s->code, s->open_scan, s->split_scan, n_words, src_words,
                                                                 uint32_t(p->n_words + 8 * splits), s->list_word + off, s->gbase[nx], s->gkey[nx],
                                                                 s->gvirt[nx], s->gsrc[nx], s->status.dev);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = s->status.read(ctx))) return rc;
        if (st[kStAlign]) return malformed(ctx, "tree", "an interior pointer at level " + std::to_string(level) + " is not a multiple of 8");
        if (st[kStRange])
            return malformed(ctx, "tree", "an interior pointer at level " + std::to_string(level) + " leaves the first n_words = " +
                                              std::to_string(p->n_words) + " words");
        if (st[kStDup]) return malformed(ctx, "tree", "a group is reached twice");  // (the marks of the level above)
        if (st[kStSrcAlign]) return malformed(ctx, "source", "an interior pointer at level " + std::to_string(level) + " is not a multiple of 8");
        if (st[kStSrcRange])
            return malformed(ctx, "source", "an interior pointer at level " + std::to_string(level) + " leaves the first src_words = " +
                                                std::to_string(p->src_words) + " words");
        const uint32_t next = st[kStNext];
        if (next > n) return svo_fail(ctx, SVO_ERR_HIP, "the next frontier's scan is out of range");  // (never: a word opens one group at the most)
        off += n;
        last_blocks = blocks, last_level = level;
        splits += st[kStSplits];
        if (next) {
            const uint32_t grid = svo_div_up(next, kThreads);
            region_mark_kernel<<<grid, kThreads, 0, ctx->stream>>>(s->gbase[nx], s->gvirt[nx], next, (uint32_t)groups_seen, cap, s->new_of, s->status.dev);
            region_check_kernel<<<grid, kThreads, 0, ctx->stream>>>(s->gbase[nx], s->gvirt[nx], next, (uint32_t)groups_seen, cap, s->new_of,
                                                                      s->status.dev);
            HIP_TRY(ctx, hipGetLastError());
            groups_seen += next;
        }
        n = 8u * next;  // (next <= the level's words <= 2^27 + n_words: no wrap)
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvPlan));

    // status: the last level's groups reached twice, and the first refused word of level `depth`
    if (last_level == depth) min_of_blocks_kernel<1><<<1, kTopThreads, 0, ctx->stream>>>(s->bad, last_blocks, s->status.dev + kStBad);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->status.copy(ctx));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStatus));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (st[kStDup]) return malformed(ctx, "tree", "a group is reached twice");
    if (last_level == depth && st[kStBad] != kNone) {
        // the refused word's cell from its group's record, and from its flags which tree goes on below it
        const uint32_t i = st[kStBad], c = i & 7u;
        uint64_t key = 0;
        uint32_t cd = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&key, s->gkey[cur ^ 1].get() + (i >> 3), sizeof key, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&cd, s->code.get() + i, sizeof cd, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2), y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u),
                       z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
        const char *who = (cd & kSceneFiner) && (cd & kSourceFiner) ? "the scene and the source are interior nodes" :
                          (cd & kSceneFiner) ? "the scene is an interior node" : "the source is an interior node";
        return svo_fail(ctx, SVO_ERR_STATE, std::string(kOpNames[p->op]) + " meets cell (" + std::to_string(x) + ", " + std::to_string(y) + ", " +
                                                std::to_string(z) + "), where " + who + " at depth " + std::to_string(depth) +
                                                ": finer there than the combine, which does not replace the subtree");
    }
    uint64_t limit = std::min<uint64_t>(ctx->capacity, kMaxWords);
    if (p->max_words) limit = std::min<uint64_t>(limit, p->max_words);
    const uint64_t new_words = p->n_words + 8 * splits;
    if (new_words > limit)
        return svo_fail(ctx, SVO_ERR_CAP, "the combined tree needs " + std::to_string(new_words) + " words, over the limit of " + std::to_string(limit) +
                                              " (max_words, the node buffer's capacity, 2^27)");

    // commit: behind every earlier write to the store (another context may have written while this one waited)
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    const uint32_t entries = (uint32_t)off;
    region_fill_kernel<<<svo_div_up(8ull * entries, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, (uint32_t)new_words, s->list_at, s->list_word,
                                                                                          s->list_fill, entries);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvFill));
    region_write_kernel<<<svo_div_up(entries, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, (uint32_t)new_words, s->list_at, s->list_word, entries);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEnd));
    if ((rc = svo_store_note_write(ctx))) return rc;
    *n_words_out = new_words;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_combine_timing(svo_ctx *ctx, float ms_out[SVO_COMBINE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->combine) return svo_fail(ctx, SVO_ERR_STATE, "no trees combined on this context yet");
    return ctx->combine->timer.read(ctx, ms_out);
}

}  // extern "C"

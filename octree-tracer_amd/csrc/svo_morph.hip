// svo_morph.hip -- one step of mathematical morphology on the tree in the node buffer: grow it by the cells
// that touch a voxel, or shrink it by the voxels that touch an empty cell, under 6, 18 or 26 neighbours.  include/svo_hip.h has
// the rule for one cell and for one word; this file applies it level by level in svo_place.hip's frame, with its frontier,
// plan, scans, check and commit.  Where a placed scene word faces up to 2 x 2 x 2 cells of a second tree, a word here faces
// the 3 x 3 x 3 cells of its own level of the scene itself: the plan never writes, so the tree is its own neighbour as it was
// before the call.
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
//   scan, check, status, commit   the placement's, with svo_frontier.h's kernels and svo_scan.h's scans; a pointer that a later
//             level follows is every interior item written into a record, checked where it is written
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_frontier.h"  // (kNone, leaf_word, region_mark_kernel, region_check_kernel, region_fill_kernel, region_write_kernel, grow_list)
#include "svo_scan.h"  // (svo_scan_u32, block_min, min_of_blocks_kernel; svo_group.h: kThreads, kEmptyWord, kMaxWords)

namespace {

constexpr uint32_t kCellBits = 21, kCellMask = (1u << kCellBits) - 1u;  // a record's cell: x << 42 | y << 21 | z
constexpr uint32_t kItems = 27, kCentre = 13;
constexpr uint32_t kItemOut = 1u;  // an item's low four bits: 0 = a scene word without its counter
// a word's flags, as svo_combine.hip's; kFiner: an interior word at level `depth`, or a leaf there that an interior item would change
enum Code : uint32_t { kOpen = 1u, kSplit = 2u, kFiner = 4u };
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStSplits, kStBad, kStWords };

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

// The rule for the n frontier words of a level.
__global__ __launch_bounds__(kThreads) void morph_plan_kernel(const uint32_t *__restrict__ words, Morph m, uint32_t level,
                                                              const uint32_t *__restrict__ gbase, const uint32_t *__restrict__ gvirt,
                                                              const uint32_t *__restrict__ gitem, uint32_t n, uint32_t *__restrict__ code,
                                                              uint32_t *__restrict__ open_scan, uint32_t *__restrict__ split_scan,
                                                              uint32_t *__restrict__ list_at, uint32_t *__restrict__ list_word,
                                                              uint32_t *__restrict__ list_fill, uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < n) {
        const uint32_t g = i >> 3, c = i & 7u, virt = gvirt[g], here = gbase[g] + c;
        const uint32_t word = virt ? virt : words[here];  // (a real group's pointer passed the check: below n_words)
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
        code[i] = cd;
        open_scan[i] = cd & kOpen;
        split_scan[i] = (cd & kSplit) >> 1;
        list_at[i] = at;
        list_word[i] = out;
        list_fill[i] = fill;
    }
    const uint32_t first_bad = block_min<kThreads>(refused);
    if (threadIdx.x == 0) bad[blockIdx.x] = first_bad;
}

// Behind the two scans: the records of the next frontier's groups with their items, the pointers of the splits and the two
// totals, as svo_place.hip's place_emit_kernel.  A pointer that is followed is checked as the discovery checks it: the
// word's own, and every interior item's.
__global__ __launch_bounds__(kThreads) void morph_emit_kernel(const uint32_t *__restrict__ words, Morph m, const uint32_t *__restrict__ gbase,
                                                              const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt,
                                                              const uint32_t *__restrict__ gitem, uint32_t n, const uint32_t *__restrict__ code,
                                                              const uint32_t *__restrict__ open_scan, const uint32_t *__restrict__ split_scan,
                                                              uint32_t n_words, uint32_t first_new, uint32_t *__restrict__ list_word,
                                                              uint32_t *__restrict__ next_base, uint64_t *__restrict__ next_key,
                                                              uint32_t *__restrict__ next_virt, uint32_t *__restrict__ next_item,
                                                              uint32_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t cd = code[i], k = open_scan[i];
    if (i == n - 1) {
        status[kStNext] = k + (cd & kOpen);
        status[kStSplits] = split_scan[i] + ((cd & kSplit) >> 1);
    }
    if (!(cd & kOpen) || k >= n) return;  // (k < n always: a word opens one group at the most)
    const uint32_t g = i >> 3, c = i & 7u, virt = gvirt[g];
    const uint64_t key = gkey[g];
    const uint32_t word = virt ? virt : words[gbase[g] + c];
    uint32_t base, next_v = 0;
    if (cd & kSplit) {
        base = first_new + 8u * split_scan[i];
        next_v = word & ~15u;
        list_word[i] = base << 4;
    } else {
        base = word >> 4;
    }
    // the word's cell and its neighbours: the cell itself is the word, a split's the constant it hands down
#pragma unroll
    for (int dx = -1; dx <= 1; dx++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dz = -1; dz <= 1; dz++) {
                if (uint32_t((dx != 0) + (dy != 0) + (dz != 0)) > m.reach) continue;  // (the same for the whole launch)
                const uint32_t item = child_item(words, gitem, g, c, dx, dy, dz);
                if (item != kItemOut && (item >> 4) < SVO_VOXEL_OFFSET) {
                    if ((item >> 4) & 7u) status[kStAlign] = 1u;  // (every writer stores the same value)
                    else if (uint64_t(item >> 4) + 8u > n_words) status[kStRange] = 1u;
                }
                next_item[size_t(kItems) * k + uint32_t(9 * (dx + 1) + 3 * (dy + 1) + dz + 1)] = item;
            }
    next_base[k] = base;
    next_virt[k] = next_v;
    const uint32_t x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2), y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u),
                   z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
    next_key[k] = uint64_t(x) << (2 * kCellBits) | uint64_t(y) << kCellBits | z;
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// Per-context workspace of the morphology (svo_ctx::morph): svo_place_state's, with 27 items per group record.  The records
// are kept for two levels at a time, the list for the whole walk.
struct svo_morph_state {
    svo_dev<uint32_t> gbase[2], gvirt[2], gitem[2];
    svo_dev<uint64_t> gkey[2];
    svo_dev<uint32_t> code, open_scan, split_scan, bad;
    svo_dev<uint32_t> list_at, list_word, list_fill;
    svo_dev<uint32_t> new_of;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_MORPH_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

namespace {

int malformed(svo_ctx *ctx, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, "malformed tree: " + why); }

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
    // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
    const uint32_t depth = p->depth, n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), cap = n_words / 8;
    const Morph morph = {p->op, p->conn == 6 ? 1u : p->conn == 18 ? 2u : 3u, depth, p->flags & SVO_MORPH_OPEN_BOUNDARY, p->colour & 0xFFFFFFu};
    if ((rc = svo_grow(ctx, (size_t)cap, &s->new_of))) return rc;
    const uint32_t *st = s->status.host();

    // the plan reads the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    HIP_TRY(ctx, s->status.zero(ctx));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0xFF, size_t(cap) * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0, sizeof(uint32_t), ctx->stream));  // the root group is group 0 of the frontiers
    if ((rc = svo_grow(ctx, 1, &s->gbase[0], &s->gvirt[0])) || (rc = svo_grow(ctx, kItems, &s->gitem[0])) || (rc = svo_grow(ctx, 1, &s->gkey[0]))) return rc;
    morph_root_kernel<<<1, 32, 0, ctx->stream>>>(s->gbase[0], s->gkey[0], s->gvirt[0], s->gitem[0]);
    HIP_TRY(ctx, hipGetLastError());

    // plan: off = the frontier words of the levels above (the list's entries so far), n = this level's
    uint64_t off = 0, groups_seen = 1, splits = 0;
    uint32_t n = 8, last_blocks = 0, last_level = 0;
    int cur = 0;
    for (uint32_t level = 1; level <= depth && n; level++, cur ^= 1) {
        // every frontier word is a word of its own of the new tree
        if (off + n > kMaxWords + 8ull * cap)
            return svo_fail(ctx, SVO_ERR_CAP, "the new tree needs more than 2^27 words, over the limit (max_words, the node buffer's capacity, 2^27)");
        const int nx = cur ^ 1;
        const uint32_t blocks = svo_div_up(n, kThreads);
        if ((rc = svo_grow(ctx, (size_t)n, &s->code, &s->open_scan, &s->split_scan)) || (rc = svo_grow(ctx, (size_t)blocks, &s->bad)) ||
            (rc = svo_grow(ctx, (size_t)n, &s->gbase[nx], &s->gvirt[nx])) || (rc = svo_grow(ctx, kItems * (size_t)n, &s->gitem[nx])) ||
            (rc = svo_grow(ctx, (size_t)n, &s->gkey[nx])) || (rc = grow_list(ctx, off + n, off, &s->list_at, &s->list_word, &s->list_fill)))
            return rc;
        morph_plan_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, morph, level, s->gbase[cur], s->gvirt[cur], s->gitem[cur], n, s->code,
                                                               s->open_scan, s->split_scan, s->list_at + off, s->list_word + off, s->list_fill + off,
                                                               s->bad);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = svo_scan_u32(ctx, s->open_scan, n)) || (rc = svo_scan_u32(ctx, s->split_scan, n))) return rc;
        morph_emit_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, morph, s->gbase[cur], s->gkey[cur], s->gvirt[cur], s->gitem[cur], n, s->code,
                                                               s->open_scan, s->split_scan, n_words, uint32_t(p->n_words + 8 * splits),
                                                               s->list_word + off, s->gbase[nx], s->gkey[nx], s->gvirt[nx], s->gitem[nx], s->status.dev);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = s->status.read(ctx))) return rc;
        if (st[kStAlign]) return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " is not a multiple of 8");
        if (st[kStRange])
            return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " leaves the first n_words = " + std::to_string(p->n_words) +
                                      " words");
        if (st[kStDup]) return malformed(ctx, "a group is reached twice");  // (the marks of the level above)
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
    if (st[kStDup]) return malformed(ctx, "a group is reached twice");
    if (last_level == depth && st[kStBad] != kNone) {
        // the refused word's cell from its group's record (the last level's records are the current ones: nothing was emitted behind them)
        const uint32_t i = st[kStBad], c = i & 7u;
        uint64_t key = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&key, s->gkey[cur ^ 1].get() + (i >> 3), sizeof key, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2), y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u),
                       z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
        return svo_fail(ctx, SVO_ERR_STATE, std::string(kOpNames[p->op]) + " meets cell (" + std::to_string(x) + ", " + std::to_string(y) + ", " +
                                                std::to_string(z) + "), where the tree is finer than depth " + std::to_string(depth) +
                                                ": the cell or a neighbour that would change it is an interior node there");
    }
    uint64_t limit = std::min<uint64_t>(ctx->capacity, kMaxWords);
    if (p->max_words) limit = std::min<uint64_t>(limit, p->max_words);
    const uint64_t new_words = p->n_words + 8 * splits;
    if (new_words > limit)
        return svo_fail(ctx, SVO_ERR_CAP, "the new tree needs " + std::to_string(new_words) + " words, over the limit of " + std::to_string(limit) +
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

int svo_morph_timing(svo_ctx *ctx, float ms_out[SVO_MORPH_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->morph) return svo_fail(ctx, SVO_ERR_STATE, "no morphology step run on this context yet");
    return ctx->morph->timer.read(ctx, ms_out);
}

}  // extern "C"

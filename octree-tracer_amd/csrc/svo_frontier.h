// svo_frontier.h -- the one home of the top-down walk that edits the tree in the node buffer, for the shape
// edit (svo_region.hip), the combine (svo_combine.hip), the placement (svo_place.hip), the affine placement
// (svo_transform.hip), the morphology step (svo_morph.hip) and the height-map edit (svo_heightmap.hip).  A pass has a plan and an emit kernel of its own, which hold its rule;
// everything around them stands here, once:
//
//   frontier  the words of a level that the pass may touch, as groups of eight: the group's first word (in the buffer, or
//             in a group that a split will make: a *virtual* group, whose eight words are one leaf word kept in the record)
//             and the cell of its parent.  Level 1 is the root group.  A pass may keep more per group, in arrays of its own
//   plan      per level, reading only, one lane per frontier word: the pass's kernel flags its word opened or split and puts
//             what it would write into the write list, which has one entry per frontier word of every level (plan_store)
//   scan      two in-place scans (svo_scan_u32) of the flags: the place of the word's children in the next frontier and
//             the number of its split among the level's; the pass's emit kernel makes the next level's records from them
//             (emit_head, emit_record), so a virtual child's address is known before anything is written.  The next
//             frontier's size and the split count come back with the status words, once per level
//   check     every group reached through a pointer marks itself in new_of; a mark found or lost is a group reached twice
//   status    the first refused word of level `depth` in frontier order (a minimum over the blocks' minima), read back with
//             its cell, for the pass's message
//   commit    a fill launch writes the eight leaf words of every new group, then one launch writes the list.  No two
//             entries name the same word
//
// svo_frontier_walk is the workspace, one per context (svo_ctx::frontier), that the six passes take turns in: nothing in
// it is read after the call that wrote it returns.  It is one type for all files.  What launches kernels is in an anonymous
// namespace like them, a copy per file: the kernels under the names they had in svo_region.hip, and Walk, one call's walk
// in that workspace.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_scan.h"  // (svo_scan_u32, block_min, min_of_blocks_kernel; svo_group.h: kThreads, kMaxWords)

// the walk's status words: the discovery's four (svo_ctx.h), the splits and the first refused word, then two of a pass's own
constexpr size_t SVO_FRONTIER_STATUS = SVO_WALK_STATUS + 4;

// Two sets of frontier records that the levels take turns in, the per-word arrays of one level, the write list of all
// levels, the marks and the status words.
struct svo_frontier_walk {
    svo_dev<uint32_t> gbase[2], gvirt[2];
    svo_dev<uint64_t> gkey[2];
    svo_dev<uint32_t> code, open_scan, split_scan, bad;
    svo_dev<uint32_t> list_at, list_word, list_fill;
    svo_dev<uint32_t> new_of;
    svo_mirrored<> status;

    int create(svo_ctx *ctx) { return status.alloc(ctx, SVO_FRONTIER_STATUS); }
};

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

__host__ __device__ inline uint32_t leaf_word(uint32_t v) { return (uint32_t(SVO_VOXEL_OFFSET) + v) << 4; }
__host__ __device__ inline bool mode_applies(uint32_t mode, uint32_t v) { return (v ? mode & SVO_REGION_VOXELS : mode & SVO_REGION_EMPTY) != 0u; }

// a word's flags.  kOpen: eight children in the next frontier; kSplit: ... of a new group.  A pass adds bits of its own above
enum Code : uint32_t { kOpen = 1u, kSplit = 2u };
// the words read back: the discovery's names for the first four (svo_ctx.h), then the walk's; a pass's own from kStWords on
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStSplits, kStBad, kStWords };
static_assert(kStWords + 2 == SVO_FRONTIER_STATUS, "the workspace's status words");

// ---- a record's cell: x << 42 | y << 21 | z, the cell of a group's parent on the parent's level ----
constexpr uint32_t kCellBits = 21, kCellMask = (1u << kCellBits) - 1u;
struct Cell {
    uint32_t x, y, z;
};
__host__ __device__ inline uint64_t cell_pack(uint32_t x, uint32_t y, uint32_t z) { return uint64_t(x) << (2 * kCellBits) | uint64_t(y) << kCellBits | z; }
__host__ __device__ inline uint32_t child_axis(uint64_t key, uint32_t shift, uint32_t bit) { return (uint32_t(key >> shift) & kCellMask) * 2u + bit; }
// the cell of child c of the cell `key`, on the child's level
__host__ __device__ inline Cell child_cell(uint64_t key, uint32_t c) {
    return {child_axis(key, 2 * kCellBits, c >> 2), child_axis(key, kCellBits, (c >> 1) & 1u), child_axis(key, 0, c & 1u)};
}

// ---- what the kernels of a level get, by value ----
// the frontier: its groups' records and its n words
struct Frontier {
    const uint32_t *gbase;
    const uint64_t *gkey;
    const uint32_t *gvirt;
    uint32_t n;
};
// The plan's outputs.  code[i] = the word's flags, also as the two scans' inputs; list_at[i] = the word's address when
// something is written there (kNone: nothing), list_word[i] = what (a split's pointer comes from the emit), list_fill[i] =
// the leaf word a split's new group is filled with; bad[block] = the block's first refused word, in frontier order.
struct PlanOut {
    uint32_t *code, *open_scan, *split_scan, *list_at, *list_word, *list_fill, *bad;
};
// The emit's: the flags and their scans, the words the scene's pointers must stay within, the first new group's address,
// the level's part of the list, the next frontier's records and the status words.
struct EmitArgs {
    const uint32_t *code, *open_scan, *split_scan;
    uint32_t n_words, first_new;
    uint32_t *list_word, *next_base;
    uint64_t *next_key;
    uint32_t *next_virt, *status;
};

// What the lane of frontier word i knows of it: where it is, the word as it stands and the word's cell on its level.
struct Entry {
    uint32_t at, word, x, y, z;
};
__device__ inline Entry frontier_entry(const uint32_t *__restrict__ words, const Frontier &f, uint32_t i) {
    const uint32_t g = i >> 3, c = i & 7u, virt = f.gvirt[g];
    const Cell cell = child_cell(f.gkey[g], c);
    Entry e;
    e.at = f.gbase[g] + c;
    e.word = virt ? virt : words[e.at];  // (a real group's pointer passed the check: below n_words)
    e.x = cell.x, e.y = cell.y, e.z = cell.z;
    return e;
}

// The end of every plan kernel: lane i's outputs ...
__device__ inline void plan_store(const PlanOut &o, uint32_t i, uint32_t cd, uint32_t at, uint32_t out, uint32_t fill) {
    o.code[i] = cd;
    o.open_scan[i] = cd & kOpen;
    o.split_scan[i] = (cd & kSplit) >> 1;
    o.list_at[i] = at;
    o.list_word[i] = out;
    o.list_fill[i] = fill;
}
// ... and, by every lane of the block, the block's first refused word (`refused`: the lane's i, or kNone).
__device__ inline void plan_refused(const PlanOut &o, uint32_t refused) {
    const uint32_t first = block_min<kThreads>(refused);
    if (threadIdx.x == 0) o.bad[blockIdx.x] = first;
}

// The head of every emit kernel, behind the two scans: the two totals into the status words, and for a lane whose word is
// opened (the others get false) its entry, the place k of its children's group in the next frontier, the group's address
// `base` and, for a split, whose groups start at first_new in the order of the scan and whose pointer goes into the list,
// the leaf word `virt` that the group is filled with.  A scene pointer that is followed is checked as the discovery checks
// it.  The caller writes what its pass keeps per group at k, then emit_record.
struct Opened {
    Entry e;
    uint32_t i, k, base, virt;
};
__device__ inline bool emit_head(const uint32_t *__restrict__ words, const Frontier &f, const EmitArgs &a, Opened &o) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, n = f.n;
    if (i >= n) return false;
    const uint32_t cd = a.code[i], k = a.open_scan[i];
    if (i == n - 1) {
        a.status[kStNext] = k + (cd & kOpen);
        a.status[kStSplits] = a.split_scan[i] + ((cd & kSplit) >> 1);
    }
    if (!(cd & kOpen) || k >= n) return false;  // (k < n always: a word opens one group at the most)
    o.e = frontier_entry(words, f, i);
    o.i = i, o.k = k, o.virt = 0;
    if (cd & kSplit) {
        o.base = a.first_new + 8u * a.split_scan[i];
        o.virt = o.e.word & ~15u;
        a.list_word[i] = o.base << 4;
    } else {
        o.base = o.e.word >> 4;
        if (o.base & 7u) a.status[kStAlign] = 1u;  // (every writer stores the same value)
        else if (uint64_t(o.base) + 8u > a.n_words) a.status[kStRange] = 1u;
    }
    return true;
}
__device__ inline void emit_record(const EmitArgs &a, const Opened &o) {
    a.next_base[o.k] = o.base;
    a.next_virt[o.k] = o.virt;
    a.next_key[o.k] = cell_pack(o.e.x, o.e.y, o.e.z);
}

// A group reached through a pointer is reached once: the groups [0, n) of a frontier, numbered from `first_id` on, mark
// themselves in new_of (kNone: not reached yet).  A mark that is there already, from an earlier level or from another lane
// of this launch, is a second path; so is a mark that another lane of this launch overwrote, which the check finds.
// status[SVO_WALK_DUP] says so.
__global__ __launch_bounds__(kThreads) void region_mark_kernel(const uint32_t *__restrict__ gbase, const uint32_t *__restrict__ gvirt, uint32_t n,
                                                               uint32_t first_id, uint32_t cap, uint32_t *new_of, uint32_t *status) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || gvirt[k] || (gbase[k] >> 3) >= cap) return;
    if (new_of[gbase[k] >> 3] != kNone) status[SVO_WALK_DUP] = 1u;
    else new_of[gbase[k] >> 3] = first_id + k;
}
__global__ __launch_bounds__(kThreads) void region_check_kernel(const uint32_t *__restrict__ gbase, const uint32_t *__restrict__ gvirt, uint32_t n,
                                                                uint32_t first_id, uint32_t cap, const uint32_t *__restrict__ new_of,
                                                                uint32_t *status) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || gvirt[k] || (gbase[k] >> 3) >= cap) return;
    if (new_of[gbase[k] >> 3] != first_id + k) status[SVO_WALK_DUP] = 1u;
}

// The commit: the eight leaf words of every new group, one lane per word ...
__global__ __launch_bounds__(kThreads) void region_fill_kernel(uint32_t *__restrict__ words, uint32_t new_words, const uint32_t *__restrict__ list_at,
                                                               const uint32_t *__restrict__ list_word, const uint32_t *__restrict__ list_fill,
                                                               uint32_t n) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x, i = t >> 3, c = t & 7u;
    if (i >= n || list_at[i] == kNone) return;
    const uint32_t pointer = list_word[i] >> 4;
    if (pointer < SVO_VOXEL_OFFSET && uint64_t(pointer) + 8u <= new_words) words[pointer + c] = list_fill[i];  // (a split's entry)
}
// ... and then the list, one lane per entry.
__global__ __launch_bounds__(kThreads) void region_write_kernel(uint32_t *__restrict__ words, uint32_t new_words, const uint32_t *__restrict__ list_at,
                                                                const uint32_t *__restrict__ list_word, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = list_at[i];
    if (at < new_words) words[at] = list_word[i];  // (kNone is not below it)
}

// room for `want` items in a list whose first `keep` items stay, at least doubled so that the levels' growth copies little
inline int grow_list(svo_ctx *ctx, size_t want, size_t keep, svo_dev<uint32_t> *a, svo_dev<uint32_t> *b, svo_dev<uint32_t> *c) {
    if (a->size() >= want) return SVO_OK;  // (the three grow together)
    want = std::max(want, 2 * a->size());
    for (svo_dev<uint32_t> *buf : {a, b, c})
        if (int rc = svo_grow_keep(ctx, want, buf, keep)) return rc;
    return SVO_OK;
}

// ---- the host frame ----

// A level as the pass's two launches see it: `blocks` workgroups of kThreads cover its n = at.n words; the records of
// its groups are set `cur` of the two, those of the next level's set `nx`, for what the pass keeps per group beside them.
struct Level {
    uint32_t level, blocks;
    int cur, nx;
    Frontier at;
    PlanOut out;
    EmitArgs emit;
};

// What a pass hands to Walk::run, a struct with these members; one that keeps nothing per group of its own and reads no
// status word of its own inherits the three below them:
//   void plan(svo_ctx *, const Level &)    its plan kernel for the level, launched on the context's stream
//   void emit(svo_ctx *, const Level &)    its emit kernel, behind the two scans
//   kWantsCode                             whether its message needs the refused word's flags
struct FrontierPass {
    static constexpr bool kWantsCode = false;
    // room for the `groups` records of set `set` in the pass's own arrays (the root's: set 0, one group)
    int grow(svo_ctx *, int, size_t) { return SVO_OK; }
    // the first frontier's one record, which has room: the root group, real, its parent the cell 0
    int root(svo_ctx *ctx, svo_frontier_walk &w) {
        HIP_TRY(ctx, hipMemsetAsync(w.gbase[0], 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(w.gvirt[0], 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(w.gkey[0], 0, sizeof(uint64_t), ctx->stream));
        return SVO_OK;
    }
    // the pass's own refusals from a level's status words, behind the walk's
    int check(svo_ctx *, const uint32_t *, uint32_t) { return SVO_OK; }
};

// One call's walk in the context's workspace.  The entry point checks its arguments, then
//   begin()   the workspace for a tree of n_words words, behind the store's last write; records `started`
//   run()     the levels with the pass's launches, the read-backs and the refusals of a malformed tree; records `planned`
//             behind the last level and `judged` behind the status words' last copy.  Afterwards `refused` says whether a
//             word of level `depth` was refused, `cell` which (the first in frontier order) and `code` its flags
//   commit()  the refusal of a tree over the limit, all before the first write; then the two launches (`filled` between
//             them, `written` behind them), the note of the write and *n_words_out
// `noun` is the tree's in the capacity messages: "edited", "combined" or "new".
struct Walk {
    svo_frontier_walk *w = nullptr;
    const char *noun = "";
    uint64_t n_words_in = 0, off = 0, splits = 0;  // off: the list's entries
    uint32_t depth = 0, n_words = 0, cap = 0;      // the words clamped to 2^27 (no pointer reaches further), the groups they hold
    bool refused = false;
    Cell cell{};
    uint32_t code = 0;

    int malformed(svo_ctx *ctx, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, "malformed tree: " + why); }

    int begin(svo_ctx *ctx, uint64_t n_words_, uint32_t depth_, const char *noun_, hipEvent_t started) {
        if (int rc = svo_workspace_ensure(ctx, ctx->frontier)) return rc;
        w = ctx->frontier.get();
        noun = noun_, n_words_in = n_words_, depth = depth_;
        // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
        n_words = (uint32_t)std::min<uint64_t>(n_words_in, kMaxWords), cap = n_words / 8;
        if (int rc = svo_grow(ctx, (size_t)cap, &w->new_of)) return rc;
        // the plan reads the words: behind every earlier write to the store, whichever context issued it
        if (int rc = svo_store_order_after_write(ctx)) return rc;
        HIP_TRY(ctx, hipEventRecord(started, ctx->stream));
        return SVO_OK;
    }

    template <class Pass>
    int run(svo_ctx *ctx, Pass &pass, hipEvent_t planned, hipEvent_t judged) {
        int rc;
        const uint32_t *st = w->status.host();
        HIP_TRY(ctx, w->status.zero(ctx));
        HIP_TRY(ctx, hipMemsetAsync(w->new_of, 0xFF, size_t(cap) * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(w->new_of, 0, sizeof(uint32_t), ctx->stream));  // the root group is group 0 of the frontiers
        if ((rc = svo_grow(ctx, 1, &w->gbase[0], &w->gvirt[0])) || (rc = svo_grow(ctx, 1, &w->gkey[0])) || (rc = pass.grow(ctx, 0, 1)) ||
            (rc = pass.root(ctx, *w)))
            return rc;
        HIP_TRY(ctx, hipGetLastError());

        // plan: off = the frontier words of the levels above (the list's entries so far), n = this level's
        uint64_t groups_seen = 1;
        uint32_t n = 8, last_blocks = 0, last_level = 0;
        int cur = 0;
        for (uint32_t level = 1; level <= depth && n; level++, cur ^= 1) {
            // every frontier word is a word of its own of the new tree
            if (off + n > kMaxWords + 8ull * cap)
                return svo_fail(ctx, SVO_ERR_CAP, std::string("the ") + noun + " tree needs more than 2^27 words, over the limit (max_words, the node buffer's capacity, 2^27)");
            const int nx = cur ^ 1;
            const uint32_t blocks = svo_div_up(n, kThreads);
            if ((rc = svo_grow(ctx, (size_t)n, &w->code, &w->open_scan, &w->split_scan)) || (rc = svo_grow(ctx, (size_t)blocks, &w->bad)) ||
                (rc = svo_grow(ctx, (size_t)n, &w->gbase[nx], &w->gvirt[nx])) || (rc = svo_grow(ctx, (size_t)n, &w->gkey[nx])) ||
                (rc = pass.grow(ctx, nx, n)) || (rc = grow_list(ctx, off + n, off, &w->list_at, &w->list_word, &w->list_fill)))
                return rc;
            const Level l = {level, blocks, cur, nx, {w->gbase[cur], w->gkey[cur], w->gvirt[cur], n},
                             {w->code, w->open_scan, w->split_scan, w->list_at + off, w->list_word + off, w->list_fill + off, w->bad},
                             {w->code, w->open_scan, w->split_scan, n_words, uint32_t(n_words_in + 8 * splits), w->list_word + off, w->gbase[nx],
                              w->gkey[nx], w->gvirt[nx], w->status.dev}};
            pass.plan(ctx, l);
            HIP_TRY(ctx, hipGetLastError());
            if ((rc = svo_scan_u32(ctx, w->open_scan, n)) || (rc = svo_scan_u32(ctx, w->split_scan, n))) return rc;
            pass.emit(ctx, l);
            HIP_TRY(ctx, hipGetLastError());
            if ((rc = w->status.read(ctx))) return rc;
            if (st[kStAlign]) return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " is not a multiple of 8");
            if (st[kStRange])
                return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " leaves the first n_words = " +
                                          std::to_string(n_words_in) + " words");
            if (st[kStDup]) return malformed(ctx, "a group is reached twice");  // (the marks of the level above)
            if ((rc = pass.check(ctx, st, level))) return rc;
            const uint32_t next = st[kStNext];
            if (next > n) return svo_fail(ctx, SVO_ERR_HIP, "the next frontier's scan is out of range");  // (never: a word opens one group at the most)
            off += n;
            last_blocks = blocks, last_level = level;
            splits += st[kStSplits];
            if (next) {
                const uint32_t grid = svo_div_up(next, kThreads);
                region_mark_kernel<<<grid, kThreads, 0, ctx->stream>>>(w->gbase[nx], w->gvirt[nx], next, (uint32_t)groups_seen, cap, w->new_of, w->status.dev);
                region_check_kernel<<<grid, kThreads, 0, ctx->stream>>>(w->gbase[nx], w->gvirt[nx], next, (uint32_t)groups_seen, cap, w->new_of,
                                                                         w->status.dev);
                HIP_TRY(ctx, hipGetLastError());
                groups_seen += next;
            }
            n = 8u * next;  // (next <= the level's words <= 2^27 + n_words: no wrap)
        }
        HIP_TRY(ctx, hipEventRecord(planned, ctx->stream));

        // status: the last level's groups reached twice, and the first refused word of level `depth`
        if (last_level == depth) min_of_blocks_kernel<1><<<1, kTopThreads, 0, ctx->stream>>>(w->bad, last_blocks, w->status.dev + kStBad);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, w->status.copy(ctx));
        HIP_TRY(ctx, hipEventRecord(judged, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (st[kStDup]) return malformed(ctx, "a group is reached twice");
        if (last_level == depth && st[kStBad] != kNone) {
            // the refused word's cell from its group's record (the last level's records are the current ones: nothing was
            // emitted behind them), and its flags when the pass's message goes by them
            const uint32_t i = st[kStBad];
            uint64_t key = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&key, w->gkey[cur ^ 1].get() + (i >> 3), sizeof key, hipMemcpyDeviceToHost, ctx->stream));
            if (Pass::kWantsCode) HIP_TRY(ctx, hipMemcpyAsync(&code, w->code.get() + i, sizeof code, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            cell = child_cell(key, i & 7u);
            refused = true;
        }
        return SVO_OK;
    }

    int commit(svo_ctx *ctx, uint64_t max_words, hipEvent_t filled, hipEvent_t written, uint64_t *n_words_out) {
        uint64_t limit = std::min<uint64_t>(ctx->capacity, kMaxWords);
        if (max_words) limit = std::min<uint64_t>(limit, max_words);
        const uint64_t new_words = n_words_in + 8 * splits;
        if (new_words > limit)
            return svo_fail(ctx, SVO_ERR_CAP, std::string("the ") + noun + " tree needs " + std::to_string(new_words) + " words, over the limit of " +
                                                  std::to_string(limit) + " (max_words, the node buffer's capacity, 2^27)");
        // behind every earlier write to the store (another context may have written while this one waited)
        if (int rc = svo_store_order_after_write(ctx)) return rc;
        const uint32_t entries = (uint32_t)off;
        region_fill_kernel<<<svo_div_up(8ull * entries, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, (uint32_t)new_words, w->list_at, w->list_word,
                                                                                             w->list_fill, entries);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(filled, ctx->stream));
        region_write_kernel<<<svo_div_up(entries, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, (uint32_t)new_words, w->list_at, w->list_word, entries);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(written, ctx->stream));
        if (int rc = svo_store_note_write(ctx)) return rc;
        *n_words_out = new_words;
        return SVO_OK;
    }
};

}  // namespace

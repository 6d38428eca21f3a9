// svo_list.hip -- the voxels of the tree in the node buffer listed on the device: the inverse of the
// builder.  One entry per voxel word reachable from group 0, in ascending Morton order of its minimum corner on the
// `depth` grid, which is the depth-first order of the tree by child index; with SVO_LIST_EXPAND a voxel above `depth`
// becomes its cells of the `depth` grid.  No sort and no atomics: counts bottom-up, offsets top-down, so the list does
// not depend on where the groups sit in the buffer or on the run.  Every tree kernel gives 8 lanes to a group, one
// word per lane (svo_group.h); sums and prefixes over a group are cross-lane operations inside its 8-lane segment.
//
//   discover  svo_tree_discover (svo_compact.hip) into the plan's svo_tree_walk: order, first_child, the levels; pointer
//             checks, the reached-twice check
//   count     bottom-up, one launch per level: cnt[k] = sum over the group's words of the entries a voxel gives (1, or
//             8^(depth - level) with expand), cnt[child] for an interior word, 0 for the empty word; rcnt[k] the same
//             for the voxels above `depth` that the expansion handles as records.  A level below `depth` only notes
//             whether it holds anything.  cnt[0], rcnt[0], those notes and the check's verdict come back in one copy:
//             the last point of failure
//   offsets   top-down, one launch per level: an exclusive prefix over the 8 lanes gives every word its start; an
//             interior word hands it to its child group with the child's Morton prefix (a leading 1, then 3 bits per
//             level: the level is the position of that 1)
//   emit      one launch over all groups: a voxel lane writes its entry at its start, or, expanded and above `depth`, its
//             record (start, key, value) at its record start: the records are sorted by start.  A second launch, one
//             lane per output entry, finds the record that covers the entry by binary search and writes the cell whose
//             Morton suffix is the entry's distance from the record's start
//
// Every error is decided before the offsets, so it leaves the outputs as they were.  The node buffer is only read.
// Discover, count and offsets stand behind svo_list_plan_count and svo_list_plan_offsets (svo_ctx.h): the surface pass
// (svo_surface.hip) runs them too, on a plan of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_group.h"   // (kThreads; group_lane: 8 lanes per group; kMaxWords)
#include "svo_morton.h"  // (morton_decode, key_bits)

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;
// the words read back: the discovery's (svo_ctx.h), the root's counts, one note per level below `depth`
enum Status { kStCountLo = SVO_WALK_STATUS, kStCountHi, kStRecords, kStPad, kStDeep, kStWords = kStDeep + 32 };

// What a word adds to its group's entry and record counts; `leaf` entries per voxel of this level, `coarse`: such a
// voxel is a record.  Every lane of the wave must get here with group_lane's result.
struct Share {
    bool voxel;
    uint64_t entries;
    uint32_t records;
};

__device__ inline Share word_share(const GroupLane &g, bool valid, uint32_t child, uint64_t leaf, uint32_t coarse, const uint64_t *cnt,
                                   const uint32_t *rcnt) {
    Share s;
    s.voxel = valid && g.pointer > SVO_VOXEL_OFFSET;
    s.entries = s.voxel ? leaf : 0u;
    s.records = s.voxel ? coarse : 0u;
    if (g.interior) {  // (valid)
        s.entries = cnt[child];
        s.records = rcnt[child];
    }
    return s;
}

// exclusive prefix of v over the 8 lanes of a group
__device__ inline uint32_t prefix8(uint32_t v, uint32_t c) {
    uint32_t inc = v;
    for (uint32_t d = 1; d < 8; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 8);
        if (c >= d) inc += t;
    }
    return inc - v;
}

// The level order[off, off + n), behind the launches of the levels below it.  With `deep` the level lies below `depth`:
// it counts nothing and notes whether it holds a voxel or an interior word (every writer stores the same value).
__global__ __launch_bounds__(kThreads) void list_count_kernel(const uint32_t *words, const uint32_t *order, uint32_t off, uint32_t n,
                                                              const uint32_t *first_child, uint64_t leaf, uint32_t coarse,
                                                              uint64_t *cnt, uint32_t *rcnt, uint32_t *deep) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const bool valid = k < n;
    const GroupLane g = group_lane(words, order + off, k, c, valid);
    uint64_t v = 0;
    uint32_t r = 0;
    if (deep) {
        if (valid && g.pointer != SVO_VOXEL_OFFSET) *deep = 1u;
    } else {
        const Share s = word_share(g, valid, g.interior ? first_child[off + k] + g.below : 0u, leaf, coarse, cnt, rcnt);
        v = s.entries;
        r = s.records;
    }
    for (uint32_t d = 1; d < 8; d <<= 1) {
        v += __shfl_xor(v, d, 8);
        r += __shfl_xor(r, d, 8);
    }
    if (valid && c == 0) {
        cnt[off + k] = v;
        rcnt[off + k] = r;
    }
}

// the root's counts into the status words; its start, record start and Morton prefix
__global__ void list_root_kernel(const uint64_t *cnt, const uint32_t *rcnt, uint32_t *status, uint32_t *start, uint32_t *rstart,
                                 uint64_t *key) {
    status[kStCountLo] = uint32_t(cnt[0]);
    status[kStCountHi] = uint32_t(cnt[0] >> 32);
    status[kStRecords] = rcnt[0];
    start[0] = 0u;
    rstart[0] = 0u;
    key[0] = 1u;
}

// The level order[off, off + n), behind the launch of the level above it: the groups below get their starts and prefixes.
__global__ __launch_bounds__(kThreads) void list_offsets_kernel(const uint32_t *words, const uint32_t *order, uint32_t off, uint32_t n,
                                                                const uint32_t *first_child, uint64_t leaf, uint32_t coarse,
                                                                const uint64_t *cnt, const uint32_t *rcnt, uint32_t *start,
                                                                uint32_t *rstart, uint64_t *key) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const bool valid = k < n;
    const GroupLane g = group_lane(words, order + off, k, c, valid);
    const uint32_t child = g.interior ? first_child[off + k] + g.below : 0u;
    const Share s = word_share(g, valid, child, leaf, coarse, cnt, rcnt);
    const uint32_t at = prefix8(uint32_t(s.entries), c), rat = prefix8(s.records, c);  // (the total is below 2^31)
    if (g.interior) {
        start[child] = start[off + k] + at;
        rstart[child] = rstart[off + k] + rat;
        key[child] = key[off + k] << 3 | c;
    }
}

struct ListOut {
    uint32_t *xyz, *value, *level;  // level may be null
    uint32_t n;                     // entries
    uint32_t *rec_start, *rec_value;
    uint64_t *rec_key;
    uint32_t n_rec;
};

__device__ inline void write_entry(const ListOut &out, uint32_t at, uint64_t cell, uint32_t bits, uint32_t depth, uint32_t value,
                                   uint32_t level) {
    uint32_t x, y, z;
    morton_decode<uint64_t>(cell, bits, x, y, z);
    const uint32_t shift = depth - bits;
    out.xyz[3ull * at] = x << shift;
    out.xyz[3ull * at + 1] = y << shift;
    out.xyz[3ull * at + 2] = z << shift;
    out.value[at] = value;
    if (out.level) out.level[at] = level;
}

// All groups of the levels 1..depth, order[0, n).
__global__ __launch_bounds__(kThreads) void list_emit_kernel(const uint32_t *words, const uint32_t *order, uint32_t n,
                                                             const uint32_t *first_child, const uint64_t *cnt, const uint32_t *rcnt,
                                                             const uint32_t *start, const uint32_t *rstart, const uint64_t *key,
                                                             uint32_t depth, bool expand, ListOut out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, k = i >> 3, c = i & 7u;
    const bool valid = k < n;
    const GroupLane g = group_lane(words, order, k, c, valid);
    const uint64_t prefix = valid ? key[k] : 1u;
    const uint32_t level = min(key_bits(prefix) + 1u, depth);  // (at most depth: deeper groups are not launched)
    const bool coarse = expand && level < depth;
    const Share s = word_share(g, valid, g.interior ? first_child[k] + g.below : 0u, expand ? 1ull << 3u * (depth - level) : 1ull,
                               coarse ? 1u : 0u, cnt, rcnt);
    const uint32_t at = prefix8(uint32_t(s.entries), c), rat = prefix8(s.records, c);
    if (!s.voxel) return;
    const uint64_t cell = prefix << 3 | c;
    const uint32_t value = g.pointer - SVO_VOXEL_OFFSET;
    if (coarse) {
        const uint32_t j = rstart[k] + rat;
        if (j < out.n_rec) {  // (always: n_rec is the root's count)
            out.rec_start[j] = start[k] + at;
            out.rec_value[j] = value;
            out.rec_key[j] = cell;
        }
    } else if (start[k] + at < out.n) {  // (always: n is the root's count)
        write_entry(out, start[k] + at, cell ^ (1ull << 3u * level), level, depth, value, level);
    }
}

// One lane per output entry: the cells of the records.  An entry that no record covers is a voxel at `depth`, written above.
__global__ __launch_bounds__(kThreads) void list_expand_kernel(uint32_t depth, ListOut out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= out.n) return;
    uint32_t lo = 0, hi = out.n_rec;  // the last record with rec_start <= i is lo - 1
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (out.rec_start[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    if (!lo) return;
    const uint64_t cell = out.rec_key[lo - 1];
    const uint32_t level = key_bits(cell), below = 3u * (depth - level), suffix = i - out.rec_start[lo - 1];
    if (suffix >= 1ull << below) return;
    write_entry(out, i, (cell ^ (1ull << 3u * level)) << below | suffix, depth, depth, out.rec_value[lo - 1], depth);
}

enum Ev { kEvStart, kEvDiscover, kEvCount, kEvOffsets, kEvEmit, kEvs };

// the entries a voxel of `level` gives, and whether it is a record of the expansion
uint64_t leaf_entries(bool expand, uint32_t depth, uint32_t level) { return expand ? 1ull << 3u * (depth - level) : 1ull; }
uint32_t coarse_records(bool expand, uint32_t depth, uint32_t level) { return expand && level < depth ? 1u : 0u; }

}  // namespace

// Per-context workspace of the listing (svo_ctx::list): its plan (svo_ctx.h: the walk's four u32 per group and seven of
// its own), four u32 per record.
struct svo_list_state {
    svo_list_plan plan;
    svo_dev<uint32_t> rec_start, rec_value;
    svo_dev<uint64_t> rec_key;
    svo_pass_timer<kEvs, SVO_LIST_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return plan.create(ctx);
    }
};

int svo_list_plan::create(svo_ctx *ctx) { return walk.create(ctx, kStWords); }

int svo_list_plan::grow(svo_ctx *ctx, size_t groups) {
    if (int rc = walk.grow(ctx, groups)) return rc;
    return svo_grow(ctx, groups, &rcnt, &start, &rstart, &cnt, &key);
}

int svo_list_plan_count(svo_ctx *ctx, svo_list_plan *s, uint64_t n_words, uint32_t depth, bool expand, hipEvent_t discovered) {
    svo_tree_walk &w = s->walk;
    const uint32_t *st = w.status.host();
    HIP_TRY(ctx, w.status.zero(ctx));

    // discover and check
    if (int rc = svo_tree_discover(ctx, n_words, &w, discovered)) return rc;
    const std::vector<uint32_t> &level_off = w.level_off;  // level l: order[level_off[l - 1], level_off[l])
    const uint32_t n_levels = (uint32_t)level_off.size() - 1;
    s->listed = std::min(n_levels, depth);

    // count
    for (uint32_t l = n_levels; l >= 1; l--) {
        const uint32_t off = level_off[l - 1], m = level_off[l] - off;
        const bool deep = l > depth;
        list_count_kernel<<<svo_div_up(8ull * m, kThreads), kThreads, 0, ctx->stream>>>(
            ctx->nodes, w.order, off, m, w.first_child, deep ? 0ull : leaf_entries(expand, depth, l),
            deep ? 0u : coarse_records(expand, depth, l), s->cnt, s->rcnt, deep ? w.status.dev + kStDeep + l : nullptr);
    }
    list_root_kernel<<<1, 1, 0, ctx->stream>>>(s->cnt, s->rcnt, w.status.dev, s->start, s->rstart, s->key);
    HIP_TRY(ctx, hipGetLastError());
    if (int rc = w.status.read(ctx)) return rc;
    if (st[SVO_WALK_DUP]) return svo_fail(ctx, SVO_ERR_STATE, "malformed tree: a group is reached twice");
    for (uint32_t l = n_levels; l > depth; l--)
        if (st[kStDeep + l])
            return svo_fail(ctx, SVO_ERR_ARG, "the tree holds a voxel or an interior word at level " + std::to_string(l) +
                                                  ", deeper than depth = " + std::to_string(depth));
    s->count = uint64_t(st[kStCountHi]) << 32 | st[kStCountLo];
    s->n_rec = st[kStRecords];
    if (s->count >= kMaxEntries)
        return svo_fail(ctx, SVO_ERR_CAP, "the list has " + std::to_string(s->count) + " entries, 2^31 or more");
    return SVO_OK;
}

int svo_list_plan_offsets(svo_ctx *ctx, svo_list_plan *s, uint32_t depth, bool expand) {
    // the levels that have listed levels below them
    const svo_tree_walk &w = s->walk;
    for (uint32_t l = 1; l < s->listed; l++) {
        const uint32_t off = w.level_off[l - 1], m = w.level_off[l] - off;
        list_offsets_kernel<<<svo_div_up(8ull * m, kThreads), kThreads, 0, ctx->stream>>>(
            ctx->nodes, w.order, off, m, w.first_child, leaf_entries(expand, depth, l), coarse_records(expand, depth, l), s->cnt,
            s->rcnt, s->start, s->rstart, s->key);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SVO_OK;
}

extern "C" {

int svo_nodes_list_voxels(svo_ctx *ctx, const svo_list_params *p, uint32_t *xyz_out_dev, uint32_t *value_out_dev,
                          uint32_t *level_out_dev, uint64_t *n_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    int rc = svo_check_flags(ctx, p->flags, SVO_LIST_EXPAND);
    if (rc || (rc = svo_check_depth(ctx, p->depth, 21))) return rc;
    if (xyz_out_dev && !value_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null value_out_dev with xyz_out_dev given");
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), depth = p->depth;
    const bool expand = p->flags & SVO_LIST_EXPAND;
    if ((rc = svo_workspace_ensure(ctx, ctx->list))) return rc;
    svo_list_state *s = ctx->list.get();
    if ((rc = s->plan.grow(ctx, n_words / 8)) || (rc = s->timer.begin(ctx))) return rc;

    // the passes read the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    if ((rc = svo_list_plan_count(ctx, &s->plan, p->n_words, depth, expand, s->timer.ev[kEvDiscover]))) return rc;
    const svo_list_plan &pl = s->plan;
    const uint64_t count = pl.count;
    const uint32_t n_rec = pl.n_rec;
    if (xyz_out_dev && count > p->max_voxels)
        return svo_fail(ctx, SVO_ERR_CAP, "the list has " + std::to_string(count) + " entries, more than max_voxels = " +
                                              std::to_string(p->max_voxels));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvCount));

    if (xyz_out_dev && count) {
        if ((rc = svo_grow(ctx, (size_t)n_rec, &s->rec_start, &s->rec_value, &s->rec_key))) return rc;
        if ((rc = svo_list_plan_offsets(ctx, &s->plan, depth, expand))) return rc;
        HIP_TRY(ctx, s->timer.mark(ctx, kEvOffsets));

        // emit
        const ListOut out{xyz_out_dev, value_out_dev, level_out_dev, (uint32_t)count, s->rec_start, s->rec_value, s->rec_key, n_rec};
        const uint32_t m = pl.walk.level_off[pl.listed];
        list_emit_kernel<<<svo_div_up(8ull * m, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, pl.walk.order, m, pl.walk.first_child, pl.cnt,
                                                                                       pl.rcnt, pl.start, pl.rstart, pl.key, depth, expand,
                                                                                       out);
        if (n_rec) list_expand_kernel<<<svo_div_up(count, kThreads), kThreads, 0, ctx->stream>>>(depth, out);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, s->timer.mark(ctx, kEvOffsets));
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEmit));
    *n_out = count;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_list_timing(svo_ctx *ctx, float ms_out[SVO_LIST_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->list) return svo_fail(ctx, SVO_ERR_STATE, "no tree listed on this context yet");
    return ctx->list->timer.read(ctx, ms_out);
}

}  // extern "C"

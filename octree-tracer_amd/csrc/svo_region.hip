// svo_region.hip -- the tree in the node buffer edited by shapes: boxes and balls filled, carved and
// painted, top-down, so that only the words along the shapes' surfaces are looked at.  include/svo_hip.h has the rule for
// one word; this file applies it level by level.  Scans instead of atomics, integers instead of floats: the words do not
// depend on the run.
//
//   frontier  the words of a level that a shape may touch, as groups of eight: the group's first word (in the buffer, or
//             in a group that a split will make: a *virtual* group, whose eight words are one leaf word kept in the record)
//             and the cell of its parent.  Level 1 is the root group
//   plan      per level, reading only, one lane per frontier word: the shapes, staged in LDS once per workgroup, are
//             classified against the word's cube from the last to the first, until one that covers the cube in SET mode ends
//             the loop; a leaf that shapes behind it touch goes through those forwards.  The lane flags its word opened or
//             split and puts what it would write into the write list, which has one entry per frontier word of every level
//   scan      two in-place scans (svo_scan_u32) of the flags: the place of the word's children in the next frontier and
//             the number of its split among the level's; the next level's records are emitted from them, so a virtual
//             child's address is known before anything is written.  The next frontier's size and the split count come back
//             with the status words, once per level
//   check     every group reached through a pointer marks itself in new_of; a mark found or lost is a group reached twice
//   status    the first refused word of level `depth` in frontier order (a minimum over the blocks' minima), read back
//   commit    a fill launch writes the eight leaf words of every new group, then one launch writes the list.  No two
//             entries name the same word
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_ctx.h"
#include "svo_frontier.h"  // (kNone, leaf_word, the mark and check kernels, the fill and write kernels, grow_list: shared with svo_combine.hip)
#include "svo_scan.h"  // (svo_scan_u32, block_min, min_of_blocks_kernel; svo_group.h: kThreads, kEmptyWord, kMaxWords)

static_assert(sizeof(svo_region_shape) == 32, "a shape is two uint4 in LDS");

namespace {

constexpr uint32_t kCellBits = 21, kCellMask = (1u << kCellBits) - 1u;  // a record's cell: x << 42 | y << 21 | z
enum Class : uint32_t { kOut, kPart, kFull };
enum Code : uint32_t { kOpen = 1u, kSplit = 2u };  // kOpen: eight children in the next frontier; kSplit: ... of a new group
// the words read back: the discovery's names for the first four (svo_ctx.h), then this pass's own
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStSplits, kStBad, kStWords };

// One axis of a ball against the cells [c0, c0 + 2^s): the distances of the farthest and the nearest cell centre from
// the ball's centre C, in half cells, squared and added up.
__host__ __device__ inline void ball_axis(uint32_t c0, uint32_t s, uint32_t C, int64_t &far, int64_t &near) {
    const int64_t lo = 2 * int64_t(c0) + 1 - int64_t(C), hi = 2 * (int64_t(c0) + (int64_t(1) << s)) - 1 - int64_t(C);  // lo <= hi
    const int64_t f = -lo > hi ? -lo : hi;
    const int64_t n = lo > 0 ? lo : hi < 0 ? -hi : (C & 1u) ? 0 : 1;
    far += f * f;
    near += n * n;
}

__host__ __device__ inline bool box_axis_out(uint32_t c0, uint32_t s, uint32_t lo, uint32_t hi) { return c0 + (1u << s) <= lo || c0 >= hi; }
__host__ __device__ inline bool box_axis_full(uint32_t c0, uint32_t s, uint32_t lo, uint32_t hi) { return lo <= c0 && c0 + (1u << s) <= hi; }

// The shape {kind | mode << 16, colour, a[0], a[1]}, {a[2], b[0], b[1], b[2]} against the cube of 2^s cells at (x, y, z).
__host__ __device__ inline uint32_t shape_class(const uint4 &p, const uint4 &q, uint32_t x, uint32_t y, uint32_t z, uint32_t s) {
    if ((p.x & 0xFFFFu) == SVO_REGION_BOX) {
        if (box_axis_out(x, s, p.z, q.y) || box_axis_out(y, s, p.w, q.z) || box_axis_out(z, s, q.x, q.w)) return kOut;
        return box_axis_full(x, s, p.z, q.y) && box_axis_full(y, s, p.w, q.z) && box_axis_full(z, s, q.x, q.w) ? kFull : kPart;
    }
    int64_t far = 0, near = 0;
    ball_axis(x, s, p.z, far, near);
    ball_axis(y, s, p.w, far, near);
    ball_axis(z, s, q.x, far, near);
    const int64_t r2 = int64_t(q.y) * int64_t(q.y);
    return near > r2 ? kOut : far <= r2 ? kFull : kPart;
}

__host__ __device__ inline bool mode_applies(uint32_t mode, uint32_t v) { return (v ? mode & SVO_REGION_VOXELS : mode & SVO_REGION_EMPTY) != 0u; }

// What the lane of frontier word i knows of it: where it is, the word as it stands and the word's cell on its level.
struct Entry {
    uint32_t at, word, x, y, z;
};
__device__ inline Entry frontier_entry(const uint32_t *__restrict__ words, const uint32_t *__restrict__ gbase, const uint64_t *__restrict__ gkey,
                                       const uint32_t *__restrict__ gvirt, uint32_t i) {
    const uint32_t g = i >> 3, c = i & 7u, virt = gvirt[g];
    const uint64_t key = gkey[g];
    Entry e;
    e.at = gbase[g] + c;
    e.word = virt ? virt : words[e.at];  // (a real group's pointer passed the check: below n_words)
    e.x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2);
    e.y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u);
    e.z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
    return e;
}

// The rule for the n frontier words of `level` (dynamic LDS: 2 * n_shapes uint4).  code[i] = the word's flags, also as
// the two scans' inputs; list_at[i] = the word's address when something is written there (kNone: nothing), list_word[i] =
// what (a split's pointer comes from region_emit_kernel), list_fill[i] = the leaf word a split's new group is filled with;
// bad[block] = the block's first word, in frontier order, that would be opened at level == depth.
__global__ __launch_bounds__(kThreads) void region_plan_kernel(const uint32_t *__restrict__ words, const uint4 *__restrict__ shapes,
                                                               uint32_t n_shapes, uint32_t depth, uint32_t level,
                                                               const uint32_t *__restrict__ gbase, const uint64_t *__restrict__ gkey,
                                                               const uint32_t *__restrict__ gvirt, uint32_t n, uint32_t *__restrict__ code,
                                                               uint32_t *__restrict__ open_scan, uint32_t *__restrict__ split_scan,
                                                               uint32_t *__restrict__ list_at, uint32_t *__restrict__ list_word,
                                                               uint32_t *__restrict__ list_fill, uint32_t *__restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) uint4 sh[];  // (behind block_min's 1 KB of static LDS: 16-byte aligned)
    for (uint32_t t = threadIdx.x; t < 2u * n_shapes; t += kThreads) sh[t] = shapes[t];
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, s = depth - level;
    uint32_t refused = kNone;
    if (i < n) {
        const Entry e = frontier_entry(words, gbase, gkey, gvirt, i);
        const uint32_t x = e.x << s, y = e.y << s, z = e.z << s;
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        // from the last shape to the first: j covers the cube in SET mode; `last` is the last shape behind j that touches it
        uint32_t j = kNone, last = kNone;
        for (uint32_t k = n_shapes; k-- > 0;) {
            const uint4 p = sh[2 * k];
            const uint32_t cls = shape_class(p, sh[2 * k + 1], x, y, z, s);
            if (cls == kOut) continue;
            if (cls == kFull && (p.x >> 16) == SVO_REGION_SET) {
                j = k;
                break;
            }
            if (last == kNone) last = k;
        }
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (!leaf) {
            if (last != kNone) {
                if (level == depth) refused = i;
                else cd = kOpen;
            } else if (j != kNone) {  // collapse
                at = e.at;
                out = leaf_word(sh[2 * j].y & 0xFFFFFFu);
            }
        } else if (j != kNone || last != kNone) {
            const uint32_t v0 = (e.word >> 4) - SVO_VOXEL_OFFSET;
            uint32_t v = j != kNone ? sh[2 * j].y & 0xFFFFFFu : v0;
            bool split = false;
            if (last != kNone)
                for (uint32_t k = j + 1u; k <= last; k++) {  // (j == kNone: from 0)
                    const uint4 p = sh[2 * k];
                    const uint32_t colour = p.y & 0xFFFFFFu;
                    if (!mode_applies(p.x >> 16, v) || colour == v) continue;
                    const uint32_t cls = shape_class(p, sh[2 * k + 1], x, y, z, s);
                    if (cls == kFull) v = colour;
                    else if (cls == kPart) {
                        split = true;
                        break;
                    }
                }
            if (split && level < depth) {  // (at level == depth nothing is PART)
                cd = kOpen | kSplit;
                at = e.at;
                fill = e.word & ~15u;
            } else if (!split && v != v0) {
                at = e.at;
                out = leaf_word(v);
            }
        }
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
// splits, whose groups start at `first_new` in the order of the scan, and the two totals.  A pointer that is followed is
// checked as the discovery checks it.
__global__ __launch_bounds__(kThreads) void region_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ gbase,
                                                               const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt, uint32_t n,
                                                               const uint32_t *__restrict__ code, const uint32_t *__restrict__ open_scan,
                                                               const uint32_t *__restrict__ split_scan, uint32_t n_words, uint32_t first_new,
                                                               uint32_t *__restrict__ list_word, uint32_t *__restrict__ next_base,
                                                               uint64_t *__restrict__ next_key, uint32_t *__restrict__ next_virt,
                                                               uint32_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t cd = code[i], k = open_scan[i];
    if (i == n - 1) {
        status[kStNext] = k + (cd & kOpen);
        status[kStSplits] = split_scan[i] + ((cd & kSplit) >> 1);
    }
    if (!(cd & kOpen) || k >= n) return;  // (k < n always: a word opens one group at the most)
    const Entry e = frontier_entry(words, gbase, gkey, gvirt, i);
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
    next_base[k] = base;
    next_virt[k] = virt;
    next_key[k] = uint64_t(e.x) << (2 * kCellBits) | uint64_t(e.y) << kCellBits | e.z;
}

// (region_mark_kernel and region_check_kernel, a group reached twice, and the commit's region_fill_kernel and
// region_write_kernel: svo_frontier.h)

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// Per-context workspace of the shape edit (svo_ctx::region): the shapes, two sets of frontier records that the levels
// take turns in, the per-word arrays of one level, the write list of all levels, and the marks.
struct svo_region_state {
    svo_pinned<uint4> shapes_host;
    svo_dev<uint4> shapes;
    svo_dev<uint32_t> gbase[2], gvirt[2];
    svo_dev<uint64_t> gkey[2];
    svo_dev<uint32_t> code, open_scan, split_scan, bad;
    svo_dev<uint32_t> list_at, list_word, list_fill;
    svo_dev<uint32_t> new_of;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_REGION_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        HIP_TRY(ctx, shapes_host.alloc(2 * SVO_REGION_MAX_SHAPES));
        HIP_TRY(ctx, shapes.alloc(2 * SVO_REGION_MAX_SHAPES));
        return status.alloc(ctx, kStWords);
    }
};

namespace {

int malformed(svo_ctx *ctx, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, "malformed tree: " + why); }

int check_shapes(svo_ctx *ctx, const svo_region_shape *shapes, size_t n, uint32_t depth) {
    const uint64_t side = 1ull << depth;
    for (size_t k = 0; k < n; k++) {
        const svo_region_shape &s = shapes[k];
        const std::string who = "shape " + std::to_string(k);
        if (s.kind != SVO_REGION_BOX && s.kind != SVO_REGION_BALL) return svo_fail(ctx, SVO_ERR_ARG, who + ": unknown kind " + std::to_string(s.kind));
        if (s.mode < 1 || s.mode > 3) return svo_fail(ctx, SVO_ERR_ARG, who + ": mode must be 1..3 (got " + std::to_string(s.mode) + ")");
        for (int a = 0; a < 3; a++) {
            if (s.kind == SVO_REGION_BOX && (s.a[a] >= s.b[a] || s.b[a] > side))
                return svo_fail(ctx, SVO_ERR_ARG, who + ": a box needs lo < hi <= 2^depth on every axis (axis " + std::to_string(a) + ": lo " +
                                                      std::to_string(s.a[a]) + ", hi " + std::to_string(s.b[a]) + ", depth " + std::to_string(depth) + ")");
            if (s.kind == SVO_REGION_BALL && s.a[a] > 2 * side)
                return svo_fail(ctx, SVO_ERR_ARG, who + ": a ball's centre lies in [0, 2^(depth+1)] half cells (axis " + std::to_string(a) + ": " +
                                                      std::to_string(s.a[a]) + ", depth " + std::to_string(depth) + ")");
        }
        if (s.kind == SVO_REGION_BALL && s.b[0] > (1u << 23))
            return svo_fail(ctx, SVO_ERR_ARG, who + ": a ball's radius is at most 2^23 half cells (got " + std::to_string(s.b[0]) + ")");
    }
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_nodes_edit_region(svo_ctx *ctx, const svo_region_shape *shapes, size_t n_shapes, const svo_region_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (n_shapes && !shapes) return svo_fail(ctx, SVO_ERR_ARG, "null shapes");
    if (n_shapes > SVO_REGION_MAX_SHAPES)
        return svo_fail(ctx, SVO_ERR_ARG, std::to_string(n_shapes) + " shapes, more than SVO_REGION_MAX_SHAPES = " + std::to_string(SVO_REGION_MAX_SHAPES));
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc || (rc = check_shapes(ctx, shapes, n_shapes, p->depth)) || (rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a shape edit cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->region))) return rc;
    svo_region_state *s = ctx->region.get();
    if (!n_shapes) {  // nothing to edit
        s->timer.none();
        *n_words_out = p->n_words;
        return SVO_OK;
    }
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
    const uint32_t depth = p->depth, n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), cap = n_words / 8;
    const uint32_t n_sh = (uint32_t)n_shapes, lds = n_sh * (uint32_t)sizeof(svo_region_shape);
    if ((rc = svo_grow(ctx, (size_t)cap, &s->new_of))) return rc;
    const uint32_t *st = s->status.host();

    // the plan reads the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    HIP_TRY(ctx, s->status.zero(ctx));
    memcpy(s->shapes_host.get(), shapes, n_shapes * sizeof(svo_region_shape));
    HIP_TRY(ctx, hipMemcpyAsync(s->shapes, s->shapes_host, n_shapes * sizeof(svo_region_shape), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0xFF, size_t(cap) * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0, sizeof(uint32_t), ctx->stream));  // the root group is group 0 of the frontiers
    if ((rc = svo_grow(ctx, 1, &s->gbase[0], &s->gvirt[0])) || (rc = svo_grow(ctx, 1, &s->gkey[0]))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(s->gbase[0], 0, sizeof(uint32_t), ctx->stream));  // level 1: the root group, real, its parent the cell 0
    HIP_TRY(ctx, hipMemsetAsync(s->gvirt[0], 0, sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->gkey[0], 0, sizeof(uint64_t), ctx->stream));

    // plan: off = the frontier words of the levels above (the list's entries so far), n = this level's
    uint64_t off = 0, groups_seen = 1, splits = 0;
    uint32_t n = 8, last_blocks = 0, last_level = 0;
    int cur = 0;
    for (uint32_t level = 1; level <= depth && n; level++, cur ^= 1) {
        // every frontier word is a word of its own of the edited tree
        if (off + n > kMaxWords + 8ull * cap)
            return svo_fail(ctx, SVO_ERR_CAP, "the edited tree needs more than 2^27 words, over the limit (max_words, the node buffer's capacity, 2^27)");
        const int nx = cur ^ 1;
        const uint32_t blocks = svo_div_up(n, kThreads);
        if ((rc = svo_grow(ctx, (size_t)n, &s->code, &s->open_scan, &s->split_scan)) || (rc = svo_grow(ctx, (size_t)blocks, &s->bad)) ||
            (rc = svo_grow(ctx, (size_t)n, &s->gbase[nx], &s->gvirt[nx])) || (rc = svo_grow(ctx, (size_t)n, &s->gkey[nx])) ||
            (rc = grow_list(ctx, off + n, off, &s->list_at, &s->list_word, &s->list_fill)))
            return rc;
        region_plan_kernel<<<blocks, kThreads, lds, ctx->stream>>>(ctx->nodes, s->shapes, n_sh, depth, level, s->gbase[cur], s->gkey[cur],
                                                                  s->gvirt[cur], n, s->code, s->open_scan, s->split_scan, s->list_at + off,
                                                                  s->list_word + off, s->list_fill + off, s->bad);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = svo_scan_u32(ctx, s->open_scan, n)) || (rc = svo_scan_u32(ctx, s->split_scan, n))) return rc;
        region_emit_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, s->gbase[cur], s->gkey[cur], s->gvirt[cur], n, s->code, s->open_scan,
                                                                s->split_scan, n_words, uint32_t(p->n_words + 8 * splits), s->list_word + off,
                                                                s->gbase[nx], s->gkey[nx], s->gvirt[nx], s->status.dev);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = s->status.read(ctx))) return rc;
        if (st[kStAlign]) return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " is not a multiple of 8");
        if (st[kStRange])
            return malformed(ctx, "an interior pointer at level " + std::to_string(level) + " leaves the first n_words = " +
                                      std::to_string(p->n_words) + " words");
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
        // the refused word's cell from its group's record, and the last shape that touches it, found again on the host
        const uint32_t i = st[kStBad], c = i & 7u;
        uint64_t key = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&key, s->gkey[cur ^ 1].get() + (i >> 3), sizeof key, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2), y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u),
                       z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
        const uint4 *sh = s->shapes_host;
        size_t k = n_shapes;
        while (k-- > 0 && shape_class(sh[2 * k], sh[2 * k + 1], x, y, z, 0) == kOut) {}
        return svo_fail(ctx, SVO_ERR_STATE, "shape " + std::to_string(k) + " meets cell (" + std::to_string(x) + ", " + std::to_string(y) + ", " +
                                                std::to_string(z) + "), which is an interior node at depth " + std::to_string(depth) +
                                                ": the tree is finer there than the edit, and the shape does not replace the subtree");
    }
    uint64_t limit = std::min<uint64_t>(ctx->capacity, kMaxWords);
    if (p->max_words) limit = std::min<uint64_t>(limit, p->max_words);
    const uint64_t new_words = p->n_words + 8 * splits;
    if (new_words > limit)
        return svo_fail(ctx, SVO_ERR_CAP, "the edited tree needs " + std::to_string(new_words) + " words, over the limit of " + std::to_string(limit) +
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

int svo_region_timing(svo_ctx *ctx, float ms_out[SVO_REGION_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->region) return svo_fail(ctx, SVO_ERR_STATE, "no tree edited by shapes on this context yet");
    return ctx->region->timer.read(ctx, ms_out);
}

}  // extern "C"

// svo_place.hip -- a tree placed into the scene at any cell offset and in any of the cube's 48 orientations: the
// combine of two trees (svo_combine.hip) without the condition that the source's cube is a cell of the scene's
// octree.  include/svo_hip.h has the rule for one word; this file applies it level by level in svo_combine.hip's frame, with
// its frontier, plan, scans, check and commit.  One thing differs: a scene word of a level faces not one source word but the
// up to 2 x 2 x 2 cells of its own size of the oriented source that its cube overlaps, its *items*.
//
//   items     one word each: OUT, a source word without its counter (a leaf: a constant, carried down as it is; an interior
//             word: a source group) or ABOVE k, the cell of size S 2^k at the origin of the source's grid, k >= 1, which holds
//             the source's cube in its corner: a word faces it only when its own cube overlaps the source's, else it is OUT.  A
//             frontier group's record holds, beside the scene's side as in svo_combine.hip, the eight items of its parent's
//             cell, 32 bytes, at jx << 2 | jy << 1 | jz; an axis with one cell leaves j = 1 unused (OUT)
//   level     which item of the parent a child's item j is a child of, and which child, is the same for every word of a
//             level: per axis t = c + h + j, the parent's item t >> 1, its child t & 1, with h = ((-offset) mod 2 z) >= z and
//             j <= two = ((-offset) mod z != 0).  The host computes h and two per level and passes them by value; a lane reads
//             its parent's items from the record by that index
//   orient    an oriented child index becomes the source's by one table of eight (bit i of the oriented index is bit perm[i]
//             of the source's, flipped with f_i), the same at every level; above the root nothing is turned, the oriented
//             source lies at the origin whatever the orientation
//   plan      per level, reading only, one lane per frontier word: its items taken together (normalised as the header says)
//             are nothing (all OUT), one constant or a subtree, and from there on the lane is the combine's
//   scan, check, status, commit   the combine's, with svo_frontier.h's kernels and svo_scan.h's scans; a followed source
//             pointer is every interior item of a word that is opened or split
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
constexpr int64_t kMaxOffset = int64_t(1) << 21;
// an item's low four bits: 0 = a source word without its counter; kItemOut; kItemAbove, with k in the bits above
constexpr uint32_t kItemOut = 1u, kItemAbove = 2u;
enum Src : uint32_t { kOut, kLeaf, kNode };  // what the items of a frontier word come to, taken together
// a word's flags, as svo_combine.hip's
enum Code : uint32_t { kOpen = 1u, kSplit = 2u, kSceneFiner = 4u, kSourceFiner = 8u };
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStSplits, kStBad, kStSrcAlign, kStSrcRange, kStWords };

// The call's constants and the level's, by value to the kernels.  child_map: three bits per oriented child index, the source's
// child index.  side: S.  cell: the level's z; h, two: its remainders, x << 2 | y << 1 | z.
struct Facing {
    uint32_t op, depth, child_map, side;
    int32_t offset[3];
    uint32_t cell, h, two;
};

// Item j (a subset of t.two's bits) of child c, the word of the level's cell (x, y, z), of the group g: the child of one of the
// eight items in the group's record.  An interior item's pointer passed the emit's check, pointer + 8 <= src_words, before this
// level was planned.
__device__ inline uint32_t child_item(const uint32_t *__restrict__ src, const uint32_t *__restrict__ gitem, const Facing &t, uint32_t g, uint32_t c,
                                      uint32_t j, uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t tx = (c >> 2) + (t.h >> 2) + (j >> 2), ty = ((c >> 1) & 1u) + ((t.h >> 1) & 1u) + ((j >> 1) & 1u), tz = (c & 1u) + (t.h & 1u) + (j & 1u);
    const uint32_t slot = (tx >> 1) << 2 | (ty >> 1) << 1 | tz >> 1, child = (tx & 1u) << 2 | (ty & 1u) << 1 | (tz & 1u);
    const uint32_t parent = gitem[8u * g + slot], tag = parent & 15u;
    if (tag == kItemOut) return kItemOut;
    if (tag == kItemAbove) {  // the child at the origin leads on, to the source's root in the end: an interior word pointing at group 0
        if (child) return kItemOut;
        const uint32_t k = parent >> 4;
        if (k == 1u) return 0u;
        // a cell above the root holds the source's cube in its corner [0, S)^3 and nothing else: a word beside that is OUT of it
        const int32_t side = int32_t(t.side), cell = int32_t(t.cell);
        if (int32_t(x) * cell - t.offset[0] >= side || int32_t(y) * cell - t.offset[1] >= side || int32_t(z) * cell - t.offset[2] >= side) return kItemOut;
        return (k - 1u) << 4 | kItemAbove;
    }
    if ((parent >> 4) >= SVO_VOXEL_OFFSET) return parent;  // a constant, carried down
    return src[(parent >> 4) + (t.child_map >> (3u * child) & 7u)] & ~15u;
}

// What the lane of frontier word i knows of it: the scene's side as in svo_combine.hip, and what its items come to.
struct Pair {
    uint32_t at, word, x, y, z, kind, b;
};
__device__ inline Pair frontier_pair(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, const Facing &t,
                                     const uint32_t *__restrict__ gbase, const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt,
                                     const uint32_t *__restrict__ gitem, uint32_t i) {
    const uint32_t g = i >> 3, c = i & 7u, virt = gvirt[g];
    const uint64_t key = gkey[g];
    Pair e;
    e.at = gbase[g] + c;
    e.word = virt ? virt : words[e.at];  // (a real group's pointer passed the check: below n_words)
    e.x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2);
    e.y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u);
    e.z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
    // normalised: OUT is the constant 0 where f(a, 0) = a; where f only asks whether b is set, every b != 0 is one value
    const bool out_is_zero = t.op <= SVO_COMBINE_CARVE, one_value = t.op == SVO_COMBINE_CARVE || t.op == SVO_COMBINE_KEEP;
    uint32_t outs = 0, nodes = 0, constants = 0, value = 0, differ = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        if (j & ~t.two) continue;  // (the same for the whole launch)
        const uint32_t item = child_item(src, gitem, t, g, c, j, e.x, e.y, e.z), tag = item & 15u, field = item >> 4;
        uint32_t v = 0;
        if (tag == kItemOut) {
            if (!out_is_zero) {
                outs++;
                continue;
            }
        } else if (tag == kItemAbove || field < SVO_VOXEL_OFFSET) {
            nodes++;
            continue;
        } else {
            v = field - SVO_VOXEL_OFFSET;
            if (one_value) v = v != 0u;
        }
        if (constants) differ |= uint32_t(v != value);
        else value = v;
        constants++;
    }
    e.b = 0;
    if (nodes || differ || (outs && constants)) e.kind = kNode;
    else if (constants) e.kind = kLeaf, e.b = value;
    else e.kind = kOut;
    return e;
}

// The first frontier: the scene's root group, real, its parent the cell 0, whose items are OUT but for the one (if any) that
// holds the source's cube.
__global__ __launch_bounds__(8) void place_root_kernel(uint32_t *__restrict__ gbase, uint64_t *__restrict__ gkey, uint32_t *__restrict__ gvirt,
                                                       uint32_t *__restrict__ gitem, uint32_t live, uint32_t item) {
    const uint32_t j = threadIdx.x;
    if (j == 0) gbase[0] = 0u, gvirt[0] = 0u, gkey[0] = 0ull;
    if (j < 8u) gitem[j] = j == live ? item : kItemOut;
}

// The rule for the n frontier words of a level: svo_combine.hip's combine_plan_kernel behind the items.
__global__ __launch_bounds__(kThreads) void place_plan_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Facing t, uint32_t level,
                                                              const uint32_t *__restrict__ gbase, const uint64_t *__restrict__ gkey,
                                                              const uint32_t *__restrict__ gvirt, const uint32_t *__restrict__ gitem, uint32_t n,
                                                              uint32_t *__restrict__ code, uint32_t *__restrict__ open_scan,
                                                              uint32_t *__restrict__ split_scan, uint32_t *__restrict__ list_at,
                                                              uint32_t *__restrict__ list_word, uint32_t *__restrict__ list_fill,
                                                              uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t refused = kNone;
    if (i < n) {
        const Pair e = frontier_pair(words, src, t, gbase, gkey, gvirt, gitem, i);
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        const uint32_t a = leaf ? (e.word >> 4) - SVO_VOXEL_OFFSET : 0u;
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (e.kind == kLeaf) {
            if (leaf) {
                const uint32_t v = combine_value(t.op, a, e.b);
                if (v != a) at = e.at, out = leaf_word(v);
            } else {
                const uint32_t whole = whole_subtree(t.op, e.b != 0u);
                if (whole == kConstant) at = e.at, out = leaf_word(whole_constant(t.op, e.b));  // collapse
                else if (whole == kOpenIt) cd = level == t.depth ? kSceneFiner : kOpen;
            }
        } else if (e.kind == kNode) {
            if (!leaf) cd = level == t.depth ? kSceneFiner | kSourceFiner : kOpen;
            else if (!leaf_stays(t.op, a != 0u)) {
                if (level == t.depth) cd = kSourceFiner;
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

// Behind the two scans: the records of the next frontier's groups with their eight items, the pointers of the splits and the
// two totals, as svo_combine.hip's combine_emit_kernel.  A pointer that is followed is checked as the discovery checks it: the
// scene's, and every interior item's.
__global__ __launch_bounds__(kThreads) void place_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ src, Facing t,
                                                              const uint32_t *__restrict__ gbase, const uint64_t *__restrict__ gkey,
                                                              const uint32_t *__restrict__ gvirt, const uint32_t *__restrict__ gitem, uint32_t n,
                                                              const uint32_t *__restrict__ code, const uint32_t *__restrict__ open_scan,
                                                              const uint32_t *__restrict__ split_scan, uint32_t n_words, uint32_t src_words,
                                                              uint32_t first_new, uint32_t *__restrict__ list_word, uint32_t *__restrict__ next_base,
                                                              uint64_t *__restrict__ next_key, uint32_t *__restrict__ next_virt,
                                                              uint32_t *__restrict__ next_item, uint32_t *__restrict__ status) {
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
        if (base & 7u) status[kStAlign] = 1u;  // (every writer stores the same value)
        else if (uint64_t(base) + 8u > n_words) status[kStRange] = 1u;
    }
    const uint32_t x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2), y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u),
                   z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        uint32_t item = kItemOut;
        if (!(j & ~t.two)) {
            item = child_item(src, gitem, t, g, c, j, x, y, z);
            if (!(item & 15u) && (item >> 4) < SVO_VOXEL_OFFSET) {
                if ((item >> 4) & 7u) status[kStSrcAlign] = 1u;
                else if (uint64_t(item >> 4) + 8u > src_words) status[kStSrcRange] = 1u;
            }
        }
        next_item[8u * k + j] = item;
    }
    next_base[k] = base;
    next_virt[k] = next_v;
    next_key[k] = uint64_t(x) << (2 * kCellBits) | uint64_t(y) << kCellBits | z;
}

enum Ev { kEvStart, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

// (-offset) mod m, m a power of two
inline uint32_t minus_mod(int32_t offset, uint32_t m) { return uint32_t(-int64_t(offset)) & (m - 1u); }

}  // namespace

// Per-context workspace of the placement (svo_ctx::place): svo_combine_state's, with eight items per group record.
struct svo_place_state {
    svo_dev<uint32_t> gbase[2], gvirt[2], gitem[2];
    svo_dev<uint64_t> gkey[2];
    svo_dev<uint32_t> code, open_scan, split_scan, bad;
    svo_dev<uint32_t> list_at, list_word, list_fill;
    svo_dev<uint32_t> new_of;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_PLACE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

namespace {

int malformed(svo_ctx *ctx, const char *which, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, std::string("malformed ") + which + ": " + why); }

const char *const kOpNames[] = {"over", "under", "paint", "carve", "keep", "replace"};
const uint8_t kPerms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// three bits per oriented child index r: the source's child index q, bit of q[perm[i]] = bit of r[i] ^ f_i
uint32_t child_map_of(uint32_t orient) {
    const uint8_t *perm = kPerms[orient >> 3];
    uint32_t map = 0;
    for (uint32_t r = 0; r < 8; r++) {
        uint32_t q = 0;
        for (uint32_t i = 0; i < 3; i++) {
            const uint32_t bit = ((r >> (2 - i)) ^ (orient >> (2 - i))) & 1u;
            q |= bit << (2 - perm[i]);
        }
        map |= q << (3 * r);
    }
    return map;
}

}  // namespace

extern "C" {

int svo_nodes_place(svo_ctx *ctx, const uint32_t *src_dev, const svo_place_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if (!src_dev) return svo_fail(ctx, SVO_ERR_ARG, "null source");
    if (p->op > SVO_COMBINE_REPLACE) return svo_fail(ctx, SVO_ERR_ARG, "op must be 0..5 (got " + std::to_string(p->op) + ")");
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (p->src_depth < 1 || p->src_depth > p->depth)
        return svo_fail(ctx, SVO_ERR_ARG, "src_depth must be 1..depth (got " + std::to_string(p->src_depth) + ", depth " + std::to_string(p->depth) + ")");
    if (p->orient >= SVO_PLACE_ORIENTS) return svo_fail(ctx, SVO_ERR_ARG, "orient must be 0..47 (got " + std::to_string(p->orient) + ")");
    for (int a = 0; a < 3; a++)
        if (p->offset[a] < -kMaxOffset || p->offset[a] > kMaxOffset)
            return svo_fail(ctx, SVO_ERR_ARG, "offset must lie in [-2^21, 2^21] on every axis (axis " + std::to_string(a) + ": " + std::to_string(p->offset[a]) + ")");
    if ((rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a placement cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    if (p->src_words < 8 || p->src_words % 8 || p->src_words > kMaxWords)
        return svo_fail(ctx, SVO_ERR_ARG, "src_words must be a positive multiple of 8, at most 2^27 (got " + std::to_string(p->src_words) + ")");
    if (src_dev < ctx->nodes + ctx->capacity && ctx->nodes < src_dev + p->src_words)
        return svo_fail(ctx, SVO_ERR_ARG, "the source overlaps the node buffer: the scene is edited in place, so the source must be a buffer of its own");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->place))) return rc;
    svo_place_state *s = ctx->place.get();
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
    const uint32_t depth = p->depth, n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), cap = n_words / 8;
    const uint32_t src_words = (uint32_t)p->src_words;
    Facing facing = {p->op, depth, child_map_of(p->orient), 1u << p->src_depth, {p->offset[0], p->offset[1], p->offset[2]}, 0u, 0u, 0u};
    if ((rc = svo_grow(ctx, (size_t)cap, &s->new_of))) return rc;
    const uint32_t *st = s->status.host();

    // the root group's record: of the items of the whole scene cube, cells of 2^depth >= S, the one at the origin of the
    // source's grid holds the source's cube: ABOVE depth - src_depth, or the root itself
    uint32_t live = 0;  // its index in the record; 8: none, the source lies wholly outside
    for (int a = 0; a < 3; a++) {
        const int64_t first = -int64_t(p->offset[a]) >> depth;  // floor((-offset) / 2^depth): the axis' first cell, and the next when there are two
        const bool two = minus_mod(p->offset[a], 1u << depth) != 0u;
        if (first == -1 && two) live |= 4u >> a;
        else if (first != 0) live |= 8u;
    }
    live = std::min(live, 8u);
    const uint32_t above = depth - p->src_depth;

    // the plan reads the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    HIP_TRY(ctx, s->status.zero(ctx));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0xFF, size_t(cap) * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->new_of, 0, sizeof(uint32_t), ctx->stream));  // the root group is group 0 of the frontiers
    if ((rc = svo_grow(ctx, 1, &s->gbase[0], &s->gvirt[0])) || (rc = svo_grow(ctx, 8, &s->gitem[0])) || (rc = svo_grow(ctx, 1, &s->gkey[0]))) return rc;
    place_root_kernel<<<1, 8, 0, ctx->stream>>>(s->gbase[0], s->gkey[0], s->gvirt[0], s->gitem[0], live, above ? above << 4 | kItemAbove : 0u);
    HIP_TRY(ctx, hipGetLastError());

    // plan: off = the frontier words of the levels above (the list's entries so far), n = this level's
    uint64_t off = 0, groups_seen = 1, splits = 0;
    uint32_t n = 8, last_blocks = 0, last_level = 0;
    int cur = 0;
    for (uint32_t level = 1; level <= depth && n; level++, cur ^= 1) {
        // every frontier word is a word of its own of the combined tree
        if (off + n > kMaxWords + 8ull * cap)
            return svo_fail(ctx, SVO_ERR_CAP, "the combined tree needs more than 2^27 words, over the limit (max_words, the node buffer's capacity, 2^27)");
        const int nx = cur ^ 1;
        const uint32_t blocks = svo_div_up(n, kThreads), z = 1u << (depth - level);
        facing.cell = z, facing.h = facing.two = 0;
        for (int a = 0; a < 3; a++) {
            const uint32_t rem = minus_mod(p->offset[a], 2u * z);
            facing.h |= uint32_t(rem >= z) << (2 - a);
            facing.two |= uint32_t((rem & (z - 1u)) != 0u) << (2 - a);
        }
        if ((rc = svo_grow(ctx, (size_t)n, &s->code, &s->open_scan, &s->split_scan)) || (rc = svo_grow(ctx, (size_t)blocks, &s->bad)) ||
            (rc = svo_grow(ctx, (size_t)n, &s->gbase[nx], &s->gvirt[nx])) || (rc = svo_grow(ctx, 8 * (size_t)n, &s->gitem[nx])) ||
            (rc = svo_grow(ctx, (size_t)n, &s->gkey[nx])) || (rc = grow_list(ctx, off + n, off, &s->list_at, &s->list_word, &s->list_fill)))
            return rc;
        place_plan_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src_dev, facing, level, s->gbase[cur], s->gkey[cur], s->gvirt[cur],
                                                               s->gitem[cur], n, s->code, s->open_scan, s->split_scan, s->list_at + off,
                                                               s->list_word + off, s->list_fill + off, s->bad);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = svo_scan_u32(ctx, s->open_scan, n)) || (rc = svo_scan_u32(ctx, s->split_scan, n))) return rc;
        place_emit_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, src_dev, facing, s->gbase[cur], s->gkey[cur], s->gvirt[cur], s->gitem[cur], n,
                                                               s->code, s->open_scan, s->split_scan, n_words, src_words,
                                                               uint32_t(p->n_words + 8 * splits), s->list_word + off, s->gbase[nx], s->gkey[nx],
                                                               s->gvirt[nx], s->gitem[nx], s->status.dev);
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
                                                ": finer there than the placement, which does not replace the subtree");
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

int svo_place_timing(svo_ctx *ctx, float ms_out[SVO_PLACE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->place) return svo_fail(ctx, SVO_ERR_STATE, "no tree placed on this context yet");
    return ctx->place->timer.read(ctx, ms_out);
}

}  // extern "C"

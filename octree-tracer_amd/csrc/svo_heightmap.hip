// svo_heightmap.hip -- the tree in the node buffer shaped by a height map: per column of a rectangle the
// cells below the ground are filled in layers and the cells above it carved, filled or painted, top-down, so that only
// the words along the ground's surface are looked at.  include/svo_hip.h has the rule for one word; this file applies it
// level by level with the frontier, the scans, the check and the commit of the shape edit (svo_region.hip,
// svo_frontier.h).  What differs is the plan: where the shape edit classifies a cube against every shape, this one asks
// for the lowest and the highest ground under the cube's footprint, one lookup in a min/max pyramid over the map.
//
//   pyramid   level s >= 1 holds one (min, max) pair per octree-aligned tile of 2^s x 2^s columns that meets the map's
//             rectangle, tz fastest; level 0 is the map itself, clamped where it is read.  One launch makes up to six
//             levels: a lane loads a block of 4 x 4 entries (of the map: four loads of 16 bytes along z where the rows allow
//             it) and reduces it to two levels in registers, two more come from cross-lane moves inside the wave, two from
//             the sixteen pairs that the four waves leave in LDS.  A workgroup is a tile of 64 x 64 entries, aligned in the
//             scene's coordinates; what lies outside the rectangle contributes the identity (min ~0, max 0).  The next
//             launch starts from the sixth level.  Every height is read once; no atomics
//   plan      per level, reading only, one lane per frontier word: the word's cube against the extremes of its footprint
//             (heightmap_plan_kernel), then the two scans, the emit, the mark and the check as in the shape edit
//   status    the first refused word of level `depth` in frontier order, read back
//   commit    region_fill_kernel, region_write_kernel (svo_frontier.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_frontier.h"  // (kNone, leaf_word, the mark and check kernels, the fill and write kernels, grow_list)
#include "svo_scan.h"  // (svo_scan_u32, block_min, min_of_blocks_kernel; svo_group.h: kThreads, kEmptyWord, kMaxWords)

static_assert(sizeof(svo_heightmap_layer) == 8 && sizeof(svo_heightmap_params) == 120, "the header's layout");

namespace {

constexpr uint32_t kCellBits = 21, kCellMask = (1u << kCellBits) - 1u;  // a record's cell: x << 42 | y << 21 | z
enum Code : uint32_t { kOpen = 1u, kSplit = 2u };  // kOpen: eight children in the next frontier; kSplit: ... of a new group
enum Status { kStAlign = SVO_WALK_ALIGN, kStRange = SVO_WALK_RANGE, kStNext = SVO_WALK_NEXT, kStDup = SVO_WALK_DUP, kStSplits, kStBad, kStWords };

constexpr uint32_t kPyrLevels = 6;  // levels per pyramid launch: two in registers, two across lanes, two through LDS
constexpr uint32_t kPyrTile = 64;   // entries of the input level along each axis of a workgroup's tile
enum PyrMode { kPyrMap, kPyrMapVec, kPyrPairs };  // the input: the map by single heights, by four along z, a level's pairs

// One level of the pyramid: its entries are the tiles [x0, x0 + nx) x [z0, z0 + nz) of its own grid, tz fastest.  Level 0
// is the map (p: the heights, x0 and z0 the origin, nx and nz the size), every other level (min, max) pairs.
struct PyrLevel {
    void *p;
    uint32_t x0, z0, nx, nz;
};
struct PyrArgs {
    PyrLevel in, out[kPyrLevels];  // (a level that the launch does not make has nx = nz = 0)
    uint32_t clamp;                // 2^depth
};

__device__ inline void pyr_put(const PyrLevel &l, uint32_t x, uint32_t z, uint32_t lo, uint32_t hi) {
    const uint32_t xi = x - l.x0, zi = z - l.z0;  // (a tile in front of the range wraps to a large number)
    if (xi < l.nx && zi < l.nz) static_cast<uint2 *>(l.p)[size_t(xi) * l.nz + zi] = make_uint2(lo, hi);
}

// The levels a.out[0 .. 5] from the level a.in: the grid is the tiles of kPyrTile x kPyrTile input entries that the
// input's range meets, z along blockIdx.x.  Lane t holds the entries (4 (t >> 4) + r, 4 (t & 15) + c) of its tile: a wave
// is 16 rows of the tile, and a row's 16 lanes read 256 contiguous bytes of the map.
template <int kMode>
__global__ __launch_bounds__(kThreads) void heightmap_pyramid_kernel(PyrArgs a) {
    __shared__ uint2 top[16];  // the workgroup's 4 x 4 entries of the fourth level
    const uint32_t t = threadIdx.x, zq = t & 15u, xr = t >> 4;
    const uint32_t bx = (a.in.x0 / kPyrTile) + blockIdx.y, bz = (a.in.z0 / kPyrTile) + blockIdx.x;
    const uint32_t x = bx * kPyrTile + 4u * xr, z = bz * kPyrTile + 4u * zq;
    uint32_t lo[4][4], hi[4][4];
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t xi = x + r - a.in.x0;
        if (kMode == kPyrMapVec) {  // (z0 and nz are multiples of 4: the four columns are inside together)
            const uint32_t zi = z - a.in.z0;
            const bool in = xi < a.in.nx && zi < a.in.nz;
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (in) q = *reinterpret_cast<const uint4 *>(static_cast<const uint32_t *>(a.in.p) + size_t(xi) * a.in.nz + zi);
            const uint32_t h[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) lo[r][c] = in ? min(h[c], a.clamp) : kNone, hi[r][c] = in ? min(h[c], a.clamp) : 0u;
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) {
                const uint32_t zi = z + c - a.in.z0;
                const bool in = xi < a.in.nx && zi < a.in.nz;
                lo[r][c] = kNone, hi[r][c] = 0u;
                if (in && kMode == kPyrMap) lo[r][c] = hi[r][c] = min(static_cast<const uint32_t *>(a.in.p)[size_t(xi) * a.in.nz + zi], a.clamp);
                if (in && kMode == kPyrPairs) {
                    const uint2 e = static_cast<const uint2 *>(a.in.p)[size_t(xi) * a.in.nz + zi];
                    lo[r][c] = e.x, hi[r][c] = e.y;
                }
            }
        }
    }
    // registers: the lane's 2 x 2 entries of the first level and its one entry of the second
    uint32_t l2 = kNone, h2 = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 2; i++)
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t l1 = min(min(lo[2 * i][2 * k], lo[2 * i][2 * k + 1]), min(lo[2 * i + 1][2 * k], lo[2 * i + 1][2 * k + 1]));
            const uint32_t h1 = max(max(hi[2 * i][2 * k], hi[2 * i][2 * k + 1]), max(hi[2 * i + 1][2 * k], hi[2 * i + 1][2 * k + 1]));
            pyr_put(a.out[0], x / 2u + i, z / 2u + k, l1, h1);
            l2 = min(l2, l1), h2 = max(h2, h1);
        }
    pyr_put(a.out[1], x / 4u, z / 4u, l2, h2);
    // across lanes: the lane's bits 0 and 4 are the low bits of zq and xr, its bits 1 and 5 the next ones.  Every lane
    // of the wave is here
    uint32_t l3 = min(l2, (uint32_t)__shfl_xor((int)l2, 1)), h3 = max(h2, (uint32_t)__shfl_xor((int)h2, 1));
    l3 = min(l3, (uint32_t)__shfl_xor((int)l3, 16)), h3 = max(h3, (uint32_t)__shfl_xor((int)h3, 16));
    if (!(zq & 1u) && !(xr & 1u)) pyr_put(a.out[2], x / 8u, z / 8u, l3, h3);
    uint32_t l4 = min(l3, (uint32_t)__shfl_xor((int)l3, 2)), h4 = max(h3, (uint32_t)__shfl_xor((int)h3, 2));
    l4 = min(l4, (uint32_t)__shfl_xor((int)l4, 32)), h4 = max(h4, (uint32_t)__shfl_xor((int)h4, 32));
    if (!(zq & 3u) && !(xr & 3u)) {
        pyr_put(a.out[3], x / 16u, z / 16u, l4, h4);
        top[(xr / 4u) * 4u + zq / 4u] = make_uint2(l4, h4);
    }
    __syncthreads();  // (no lane has left: what is outside the rectangle was the identity)
    // LDS: four lanes take a quarter of the sixteen pairs each, the first one all of them
    if (t < 4u) {
        uint32_t l5 = kNone, h5 = 0u, l6 = kNone, h6 = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint2 e = top[k];
            l6 = min(l6, e.x), h6 = max(h6, e.y);
            if ((k / 8u) == (t >> 1) && ((k / 2u) & 1u) == (t & 1u)) l5 = min(l5, e.x), h5 = max(h5, e.y);
        }
        pyr_put(a.out[4], bx * 2u + (t >> 1), bz * 2u + (t & 1u), l5, h5);
        if (t == 0u) pyr_put(a.out[5], bx, bz, l6, h6);
    }
}

// What the plan knows of the call: the rectangle, the modes, the layers' colours and the running sums of their
// thicknesses, T[k] saturated at 2^32 - 1 (a depth below the ground is less) and T[n_layers - 1 ..] = 2^32 - 1: the last
// layer reaches down to y = 0.  `at` is the pyramid's level s = depth - level.
struct PlanArgs {
    PyrLevel at;
    uint32_t depth, level, clamp;
    uint32_t ox, oz, sx, sz;
    uint32_t mode_below, mode_above, colour_above;
    uint32_t colour[SVO_HEIGHTMAP_MAX_LAYERS], T[SVO_HEIGHTMAP_MAX_LAYERS];
};

__host__ __device__ inline bool mode_applies(uint32_t mode, uint32_t v) { return (v ? mode & SVO_REGION_VOXELS : mode & SVO_REGION_EMPTY) != 0u; }

// the layer of the cell d cells below the ground's top cell: the first k with d < T[k]
__device__ inline uint32_t band(const PlanArgs &a, uint32_t d) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t j = 0; j < SVO_HEIGHTMAP_MAX_LAYERS - 1; j++) k += d >= a.T[j] ? 1u : 0u;  // (T does not decrease)
    return k;
}

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

// The rule for the n frontier words of a.level; the outputs are region_plan_kernel's: code[i] = the word's flags, also as
// the two scans' inputs; list_at[i] = the word's address when something is written there (kNone: nothing), list_word[i] =
// what (a split's pointer comes from heightmap_emit_kernel), list_fill[i] = the leaf word a split's new group is filled
// with; bad[block] = the block's first word, in frontier order, that would be opened at level == depth.
__global__ __launch_bounds__(kThreads) void heightmap_plan_kernel(const uint32_t *__restrict__ words, PlanArgs a, const uint32_t *__restrict__ gbase,
                                                                  const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gvirt, uint32_t n,
                                                                  uint32_t *__restrict__ code, uint32_t *__restrict__ open_scan,
                                                                  uint32_t *__restrict__ split_scan, uint32_t *__restrict__ list_at,
                                                                  uint32_t *__restrict__ list_word, uint32_t *__restrict__ list_fill,
                                                                  uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, s = a.depth - a.level, S = 1u << s;
    uint32_t refused = kNone;
    if (i < n) {
        const Entry e = frontier_entry(words, gbase, gkey, gvirt, i);
        const uint32_t x0 = e.x << s, y0 = e.y << s, z0 = e.z << s;
        const bool leaf = (e.word >> 4) >= SVO_VOXEL_OFFSET;
        // the footprint meets the rectangle iff its tile is one of the level's entries
        const uint32_t xi = e.x - a.at.x0, zi = e.z - a.at.z0;
        const bool meets = xi < a.at.nx && zi < a.at.nz;
        const bool inside = x0 >= a.ox && x0 + S <= a.ox + a.sx && z0 >= a.oz && z0 + S <= a.oz + a.sz;
        uint32_t cd = 0, at = kNone, out = 0, fill = 0;
        if (meets) {
            uint32_t hmin, hmax;
            if (s == 0u) hmin = hmax = min(static_cast<const uint32_t *>(a.at.p)[size_t(xi) * a.at.nz + zi], a.clamp);
            else {
                const uint2 m = static_cast<const uint2 *>(a.at.p)[size_t(xi) * a.at.nz + zi];
                hmin = m.x, hmax = m.y;
            }
            const uint32_t k_lo = band(a, hmin > y0 + S ? hmin - y0 - S : 0u), k_hi = band(a, hmax > y0 + 1u ? hmax - 1u - y0 : 0u);
            const bool above = y0 + S > hmin && a.mode_above, below = y0 < hmax && a.mode_below;  // the candidates
            const bool all_above = y0 >= hmax, all_below = y0 + S <= hmin && k_lo == k_hi;
            const uint32_t v0 = leaf ? (e.word >> 4) - SVO_VOXEL_OFFSET : 0u;
            if (!above && !below) {
                // no candidate: the word and everything below it stay
            } else if (inside && (all_above || all_below)) {  // uniform (its one candidate's mode is not 0)
                uint32_t colour = a.colour_above & 0xFFFFFFu;
                if (!all_above)
#pragma unroll
                    for (uint32_t k = 0; k < SVO_HEIGHTMAP_MAX_LAYERS; k++)
                        if (k == k_lo) colour = a.colour[k];
                const uint32_t mode = all_above ? a.mode_above : a.mode_below;
                if (leaf) {
                    if (mode_applies(mode, v0) && colour != v0) at = e.at, out = leaf_word(colour);
                } else if (mode == SVO_REGION_SET) at = e.at, out = leaf_word(colour);  // collapse
                else if (a.level == a.depth) refused = i;
                else cd = kOpen;
            } else if (!leaf) {
                if (a.level == a.depth) refused = i;  // (never: a footprint of one column is uniform)
                else cd = kOpen;
            } else if (a.level < a.depth) {
                bool split = above && mode_applies(a.mode_above, v0) && (a.colour_above & 0xFFFFFFu) != v0;
                if (below && mode_applies(a.mode_below, v0))
#pragma unroll
                    for (uint32_t k = 0; k < SVO_HEIGHTMAP_MAX_LAYERS; k++)
                        if (k >= k_lo && k <= k_hi && a.colour[k] != v0) split = true;
                if (split) {
                    cd = kOpen | kSplit;
                    at = e.at;
                    fill = e.word & ~15u;
                }
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

// Behind the two scans, as svo_region.hip's region_emit_kernel: the records of the next frontier's groups, in the order of
// their parents, the pointers of the splits, whose groups start at `first_new` in the order of the scan, and the two
// totals.  A pointer that is followed is checked as the discovery checks it.
__global__ __launch_bounds__(kThreads) void heightmap_emit_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ gbase,
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

enum Ev { kEvStart, kEvPyramid, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// Per-context workspace of the height-map edit (svo_ctx::heightmap): the pyramid and its levels, then the shape edit's
// arrays: two sets of frontier records that the levels take turns in, the per-word arrays of one level, the write list
// of all levels, and the marks.
struct svo_heightmap_state {
    svo_dev<uint2> pyramid;
    std::vector<PyrLevel> levels;  // of the last pyramid: [0] the map, [s] the level s
    svo_dev<uint32_t> gbase[2], gvirt[2];
    svo_dev<uint64_t> gkey[2];
    svo_dev<uint32_t> code, open_scan, split_scan, bad;
    svo_dev<uint32_t> list_at, list_word, list_fill;
    svo_dev<uint32_t> new_of;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_HEIGHTMAP_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

namespace {

int malformed(svo_ctx *ctx, const std::string &why) { return svo_fail(ctx, SVO_ERR_STATE, "malformed tree: " + why); }

// the argument errors of both entry points, in the header's order
int check_params(svo_ctx *ctx, const svo_heightmap_params *p) {
    if (p->reserved) return svo_fail(ctx, SVO_ERR_ARG, "reserved must be 0 (got " + std::to_string(p->reserved) + ")");
    if (int rc = svo_check_depth(ctx, p->depth, 21)) return rc;
    if (p->mode_below > 3 || p->mode_above > 3)
        return svo_fail(ctx, SVO_ERR_ARG, "mode_below and mode_above must be 0..3 (got " + std::to_string(p->mode_below) + " and " +
                                              std::to_string(p->mode_above) + ")");
    if (p->n_layers > SVO_HEIGHTMAP_MAX_LAYERS || (p->mode_below && !p->n_layers))
        return svo_fail(ctx, SVO_ERR_ARG, "n_layers must be 0..8, and at least 1 with a mode_below (got " + std::to_string(p->n_layers) + ")");
    const uint64_t side = 1ull << p->depth;
    for (int a = 0; a < 2; a++)
        if (uint64_t(p->origin_xz[a]) + p->size_xz[a] > side)
            return svo_fail(ctx, SVO_ERR_ARG, "the map's rectangle leaves the grid: origin + size <= 2^depth on both axes (axis " + std::to_string(a) +
                                                  ": origin " + std::to_string(p->origin_xz[a]) + ", size " + std::to_string(p->size_xz[a]) + ", depth " +
                                                  std::to_string(p->depth) + ")");
    if (uint64_t(p->size_xz[0]) * p->size_xz[1] >= (1ull << 31))
        return svo_fail(ctx, SVO_ERR_ARG, "the map has 2^31 columns or more (" + std::to_string(p->size_xz[0]) + " x " + std::to_string(p->size_xz[1]) + ")");
    return SVO_OK;
}

// The pyramid of the map on the ctx stream, all levels 1..depth, into the workspace: s->levels says where they are.
int build_pyramid(svo_ctx *ctx, svo_heightmap_state *s, const svo_heightmap_params *p, const uint32_t *heights_dev) {
    const uint32_t depth = p->depth, ox = p->origin_xz[0], oz = p->origin_xz[1], sx = p->size_xz[0], sz = p->size_xz[1];
    std::vector<PyrLevel> &lv = s->levels;
    lv.assign(depth + 1, PyrLevel{});
    lv[0] = {const_cast<uint32_t *>(heights_dev), ox, oz, sx, sz};
    size_t entries = 0;
    std::vector<size_t> off(depth + 1, 0);
    for (uint32_t k = 1; k <= depth; k++) {
        lv[k].x0 = ox >> k, lv[k].z0 = oz >> k;
        lv[k].nx = ((ox + sx - 1) >> k) - lv[k].x0 + 1, lv[k].nz = ((oz + sz - 1) >> k) - lv[k].z0 + 1;
        off[k] = entries;
        entries += size_t(lv[k].nx) * lv[k].nz;
    }
    if (int rc = svo_grow(ctx, entries, &s->pyramid)) return rc;
    for (uint32_t k = 1; k <= depth; k++) lv[k].p = s->pyramid.get() + off[k];
    const bool vec = sz % 4 == 0 && oz % 4 == 0 && reinterpret_cast<uintptr_t>(heights_dev) % 16 == 0;
    for (uint32_t from = 0; from < depth; from += kPyrLevels) {
        PyrArgs a{};
        a.in = lv[from];
        a.clamp = 1u << depth;
        for (uint32_t k = 0; k < kPyrLevels && from + 1 + k <= depth; k++) a.out[k] = lv[from + 1 + k];
        const dim3 grid((a.in.z0 + a.in.nz - 1) / kPyrTile - a.in.z0 / kPyrTile + 1, (a.in.x0 + a.in.nx - 1) / kPyrTile - a.in.x0 / kPyrTile + 1);
        if (from) heightmap_pyramid_kernel<kPyrPairs><<<grid, kThreads, 0, ctx->stream>>>(a);
        else if (vec) heightmap_pyramid_kernel<kPyrMapVec><<<grid, kThreads, 0, ctx->stream>>>(a);
        else heightmap_pyramid_kernel<kPyrMap><<<grid, kThreads, 0, ctx->stream>>>(a);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_nodes_edit_heightmap(svo_ctx *ctx, const svo_heightmap_params *p, const uint32_t *heights_dev, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    const bool nothing = !p->size_xz[0] || !p->size_xz[1] || (!p->mode_below && !p->mode_above);
    if (!heights_dev && !nothing) return svo_fail(ctx, SVO_ERR_ARG, "null heights");
    int rc = check_params(ctx, p);
    if (rc || (rc = svo_check_store(ctx))) return rc;
    if (ctx->adapt)
        return svo_fail(ctx, SVO_ERR_STATE, "a device adaptive state is attached: a height-map edit cuts subtrees off under its positions and hole stack");
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->heightmap))) return rc;
    svo_heightmap_state *s = ctx->heightmap.get();
    if (nothing) {  // nothing to edit
        s->timer.none();
        *n_words_out = p->n_words;
        return SVO_OK;
    }
    const double t0 = svo_now_ms();
    if ((rc = s->timer.begin(ctx))) return rc;
    // no pointer reaches a group behind 2^27, so the words behind it hold no reachable group
    const uint32_t depth = p->depth, n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), cap = n_words / 8;
    if ((rc = svo_grow(ctx, (size_t)cap, &s->new_of))) return rc;
    const uint32_t *st = s->status.host();

    PlanArgs plan{};
    plan.depth = depth, plan.clamp = 1u << depth;
    plan.ox = p->origin_xz[0], plan.oz = p->origin_xz[1], plan.sx = p->size_xz[0], plan.sz = p->size_xz[1];
    plan.mode_below = p->mode_below, plan.mode_above = p->mode_above, plan.colour_above = p->colour_above & 0xFFFFFFu;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < SVO_HEIGHTMAP_MAX_LAYERS; k++) {
        const bool last = k + 1 >= p->n_layers;  // the last layer's thickness is ignored; the layers behind it repeat it
        const svo_heightmap_layer &l = p->layers[p->n_layers ? std::min(k, p->n_layers - 1) : 0];
        sum += l.thickness;
        plan.T[k] = last ? kNone : (uint32_t)std::min<uint64_t>(sum, kNone);
        plan.colour[k] = p->n_layers ? l.colour & 0xFFFFFFu : 0u;
    }

    // the pyramid and the plan read the words and the map: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    if ((rc = build_pyramid(ctx, s, p, heights_dev))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvPyramid));
    HIP_TRY(ctx, s->status.zero(ctx));
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
        plan.level = level;
        plan.at = s->levels[depth - level];
        heightmap_plan_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, plan, s->gbase[cur], s->gkey[cur], s->gvirt[cur], n, s->code,
                                                                   s->open_scan, s->split_scan, s->list_at + off, s->list_word + off,
                                                                   s->list_fill + off, s->bad);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = svo_scan_u32(ctx, s->open_scan, n)) || (rc = svo_scan_u32(ctx, s->split_scan, n))) return rc;
        heightmap_emit_kernel<<<blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, s->gbase[cur], s->gkey[cur], s->gvirt[cur], n, s->code, s->open_scan,
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
        // the refused word's cell from its group's record
        const uint32_t i = st[kStBad], c = i & 7u;
        uint64_t key = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&key, s->gkey[cur ^ 1].get() + (i >> 3), sizeof key, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t x = (uint32_t(key >> (2 * kCellBits)) & kCellMask) * 2u + (c >> 2), y = (uint32_t(key >> kCellBits) & kCellMask) * 2u + ((c >> 1) & 1u),
                       z = (uint32_t(key) & kCellMask) * 2u + (c & 1u);
        return svo_fail(ctx, SVO_ERR_STATE, "the height map meets cell (" + std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(z) +
                                                "), which is an interior node at depth " + std::to_string(depth) +
                                                ": the tree is finer there than the edit, and the mode does not replace the subtree");
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

int svo_heightmap_minmax(svo_ctx *ctx, const svo_heightmap_params *p, const uint32_t *heights_dev, uint32_t s, uint32_t *minmax_out_dev) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    const bool nothing = !p->size_xz[0] || !p->size_xz[1];
    if (!heights_dev && !nothing) return svo_fail(ctx, SVO_ERR_ARG, "null heights");
    if (!minmax_out_dev && !nothing) return svo_fail(ctx, SVO_ERR_ARG, "null minmax_out");
    if (int rc = check_params(ctx, p)) return rc;
    if (s < 1 || s > p->depth) return svo_fail(ctx, SVO_ERR_ARG, "s must be 1..depth (got " + std::to_string(s) + ", depth " + std::to_string(p->depth) + ")");
    if (nothing) return SVO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = svo_workspace_ensure(ctx, ctx->heightmap)) return rc;
    svo_heightmap_state *w = ctx->heightmap.get();
    if (int rc = build_pyramid(ctx, w, p, heights_dev)) return rc;
    const PyrLevel &l = w->levels[s];
    HIP_TRY(ctx, hipMemcpyAsync(minmax_out_dev, l.p, size_t(l.nx) * l.nz * sizeof(uint2), hipMemcpyDeviceToDevice, ctx->stream));
    return SVO_OK;
}

int svo_heightmap_timing(svo_ctx *ctx, float ms_out[SVO_HEIGHTMAP_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->heightmap) return svo_fail(ctx, SVO_ERR_STATE, "no tree edited by a height map on this context yet");
    return ctx->heightmap->timer.read(ctx, ms_out);
}

}  // extern "C"

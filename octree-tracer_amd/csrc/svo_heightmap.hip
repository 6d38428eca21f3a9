// svo_heightmap.hip -- the tree in the node buffer shaped by a height map: per column of a rectangle the
// cells below the ground are filled in layers and the cells above it carved, filled or painted, top-down, so that only
// the words along the ground's surface are looked at.  include/svo_hip.h has the rule for one word; this file applies it
// level by level with the walk of svo_frontier.h.  Its own is the plan: where the shape edit (svo_region.hip)
// classifies a cube against every shape, this one asks for the lowest and the highest ground under the cube's footprint, one
// lookup in a min/max pyramid over the map.
//
//   pyramid   level s >= 1 holds one (min, max) pair per octree-aligned tile of 2^s x 2^s columns that meets the map's
//             rectangle, tz fastest; level 0 is the map itself, clamped where it is read.  One launch makes up to six
//             levels: a lane loads a block of 4 x 4 entries (of the map: four loads of 16 bytes along z where the rows allow
//             it) and reduces it to two levels in registers, two more come from cross-lane moves inside the wave, two from
//             the sixteen pairs that the four waves leave in LDS.  A workgroup is a tile of 64 x 64 entries, aligned in the
//             scene's coordinates; what lies outside the rectangle contributes the identity (min ~0, max 0).  The next
//             launch starts from the sixth level.  Every height is read once; no atomics
//   plan      per level, reading only, one lane per frontier word: the word's cube against the extremes of its footprint
//             (heightmap_plan_kernel)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_frontier.h"  // (the walk: Entry, PlanOut, emit_head, Walk; kNone, leaf_word, mode_applies)

static_assert(sizeof(svo_heightmap_layer) == 8 && sizeof(svo_heightmap_params) == 120, "the header's layout");

namespace {

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

// the layer of the cell d cells below the ground's top cell: the first k with d < T[k]
__device__ inline uint32_t band(const PlanArgs &a, uint32_t d) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t j = 0; j < SVO_HEIGHTMAP_MAX_LAYERS - 1; j++) k += d >= a.T[j] ? 1u : 0u;  // (T does not decrease)
    return k;
}

// The rule for the frontier words of a.level; a word that would be opened at level == depth is refused.
__global__ __launch_bounds__(kThreads) void heightmap_plan_kernel(const uint32_t *__restrict__ words, PlanArgs a, Frontier f, PlanOut o) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, s = a.depth - a.level, S = 1u << s;
    uint32_t refused = kNone;
    if (i < f.n) {
        const Entry e = frontier_entry(words, f, i);
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
        plan_store(o, i, cd, at, out, fill);
    }
    plan_refused(o, refused);
}

// Behind the two scans: the records of the next frontier's groups, in the order of their parents.
__global__ __launch_bounds__(kThreads) void heightmap_emit_kernel(const uint32_t *__restrict__ words, Frontier f, EmitArgs a) {
    Opened o;
    if (emit_head(words, f, a, o)) emit_record(a, o);
}

enum Ev { kEvStart, kEvPyramid, kEvPlan, kEvStatus, kEvFill, kEvEnd, kEvs };

}  // namespace

// What the height-map edit keeps per context beside the walk's workspace (svo_ctx::heightmap): the pyramid, its levels and
// the times.
struct svo_heightmap_state {
    svo_dev<uint2> pyramid;
    std::vector<PyrLevel> levels;  // of the last pyramid: [0] the map, [s] the level s
    svo_pass_timer<kEvs, SVO_HEIGHTMAP_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return SVO_OK;
    }
};

namespace {

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
    const uint32_t depth = p->depth;
    struct : FrontierPass {
        svo_heightmap_state *s;
        PlanArgs args{};
        void plan(svo_ctx *ctx, const Level &l) {
            args.level = l.level;
            args.at = s->levels[args.depth - l.level];
            heightmap_plan_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, args, l.at, l.out);
        }
        void emit(svo_ctx *ctx, const Level &l) { heightmap_emit_kernel<<<l.blocks, kThreads, 0, ctx->stream>>>(ctx->nodes, l.at, l.emit); }
    } pass;
    pass.s = s;
    PlanArgs &plan = pass.args;
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
    Walk walk;
    // (the pyramid reads the map behind the store's last write too)
    if ((rc = walk.begin(ctx, p->n_words, depth, "edited", s->timer.ev[kEvStart])) || (rc = build_pyramid(ctx, s, p, heights_dev))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvPyramid));
    if ((rc = walk.run(ctx, pass, s->timer.ev[kEvPlan], s->timer.ev[kEvStatus]))) return rc;
    if (walk.refused)
        return svo_fail(ctx, SVO_ERR_STATE, "the height map meets cell (" + std::to_string(walk.cell.x) + ", " + std::to_string(walk.cell.y) + ", " +
                                                std::to_string(walk.cell.z) + "), which is an interior node at depth " + std::to_string(depth) +
                                                ": the tree is finer there than the edit, and the mode does not replace the subtree");
    if ((rc = walk.commit(ctx, p->max_words, s->timer.ev[kEvFill], s->timer.ev[kEvEnd], n_words_out))) return rc;
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

// svo_surface.hip -- the visible surface of the tree in the node buffer, found on the device: for every
// voxel of the listing (svo_list.hip) which of its six faces are exposed, delivered as a mask per voxel, as the list of
// the voxels with an exposed face, or as one entry per exposed face.  The rule per face is include/svo_hip.h's: the cell
// behind the face, on the voxel's own level, is looked up by the sampler's walk; a voxel found there covers the face, the
// empty word and finer detail expose it.  No sort and no atomics: the entries keep the listing's order, so the output
// does not depend on where the groups sit in the buffer or on the run.
//
//   plan      svo_list_plan_count / svo_list_plan_offsets (svo_list.hip): the discovery with its checks, the entry
//             counts bottom-up, then every group's place in the list and its Morton prefix top-down
//   mask      one launch over all groups of the listed levels, one lane per group: the lane loads the group's 8 words
//             once.  The 12 faces between siblings are decided from those registers.  The 24 outer faces look into the 6
//             cells beside the group on the level above: the group's prefix with +-1 on one axis, in dilated-integer
//             arithmetic (svo_morton.h).  The walk to such a cell does not start at the root: the groups of a wave follow
//             each other in Morton order, so the wave walks the path of its first group once, with scalar loads, and
//             keeps it in LDS; a lane resumes where its neighbour's key leaves that path.  A walk that ends on a voxel or
//             on the empty word settles 4 faces at once; one that arrives at the neighbour group reads its 8 words.
//             Every voxel lane-slot writes (key, value, mask) at its place in the list
//   compact   svo_scan.h's tile pass over the list's mask bytes: an entry counts 1 when it is kept (a non-zero mask, or
//             every entry with SVO_SURFACE_KEEP_HIDDEN) or, for quads, its mask's popcount.  The total comes back: the
//             last point of failure
//   emit      tile_emit_kernel: the kept entries, or their faces one by one, at their ranks
//
// No pointer is checked here: the walks start at groups on the path of a discovered group and follow only words of groups
// they reached that way, and the discovery has checked every pointer in every reachable group before the mask pass runs.
// Every error is decided before the emit, so it leaves the outputs as they were.  The node buffer is only read.
// svo_surface_list_quads (svo_ctx.h) runs the same pass for the merge (svo_surface_merge.hip), in a workspace of the merge's
// own, and leaves the quads there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_group.h"   // (kThreads, kMaxWords)
#include "svo_morton.h"  // (key_bits, morton_axis_mask, morton_step, morton_decode)
#include "svo_scan.h"    // (the tile pass)

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPathLevels = 21;  // a group's prefix holds at most 20 levels: the groups of the levels 1..21 on a path
constexpr uint32_t kKept = 0x40u;     // in a mask byte of the compaction: the entry is listed whatever its mask
enum Status { kStTotal, kStWords };
enum Mode { kModeSurface, kModeAll, kModeQuads };
static_assert(kThreads % 64 == 0, "whole waves per workgroup");

// bit c: the word is a voxel
__device__ inline uint32_t solid_mask(const uint4 &a, const uint4 &b) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) m |= (w[c] >> 4) > SVO_VOXEL_OFFSET ? 1u << c : 0u;
    return m;
}

// The groups order[0, n) of the listed levels, one lane each.  ent_*[r] gets entry r of the listing, r < n_list.
__global__ __launch_bounds__(kThreads) void surface_mask_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ order,
                                                                uint32_t n, const uint32_t *__restrict__ first_child,
                                                                const uint64_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                                const uint64_t *__restrict__ key, uint32_t closed, uint32_t n_list,
                                                                uint64_t *__restrict__ ent_key, uint32_t *__restrict__ ent_value,
                                                                uint8_t *__restrict__ ent_mask) {
    // path[w][j]: the group that j levels of the prefix of wave w's first group lead to; [0] is the root group
    __shared__ uint32_t path[kWaves][kPathLevels];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane(blockIdx.x * kThreads + wave * 64u), k = k0 + lane;
    uint64_t lead = 1u;  // the first group's prefix: the same in every lane, so its walk loads through the scalar unit
    if (k0 < n) lead = key[k0];
    const uint32_t lead_levels = key_bits(lead);
    {
        uint32_t group = 0;
        if (lane == 0) path[wave][0] = 0u;
        for (uint32_t j = 0; j < lead_levels; j++) {
            const uint32_t i = __builtin_amdgcn_readfirstlane(group + (uint32_t(lead >> 3u * (lead_levels - 1u - j)) & 7u));
            group = words[i] >> 4;  // (interior: the word lies on the path to a discovered group)
            if (lane == 0) path[wave][j + 1u] = group;
        }
    }
    __syncthreads();
    if (k >= n) return;

    const uint32_t g = order[k];  // (a multiple of 8: the group is two aligned 16-byte reads)
    const uint4 lo = *reinterpret_cast<const uint4 *>(words + g), hi = *reinterpret_cast<const uint4 *>(words + g + 4);
    const uint32_t vm = solid_mask(lo, hi);
    if (!vm) return;
    const uint32_t pointer[8] = {lo.x >> 4, lo.y >> 4, lo.z >> 4, lo.w >> 4, hi.x >> 4, hi.y >> 4, hi.z >> 4, hi.w >> 4};
    const uint64_t prefix = key[k];
    const uint32_t levels = key_bits(prefix);  // the words are of level levels + 1
    const uint64_t cell = prefix ^ (1ull << 3u * levels), lead_cell = lead ^ (1ull << 3u * lead_levels);

    // What stands in the 6 cells beside the group, as the voxel mask of a group: byte f of `beside` for face f
    uint64_t beside = 0;
    for (uint32_t f = 0; f < 6; f++) {
        const uint32_t axis = f >> 1, up = f & 1u;
        const uint32_t side = (axis == 0 ? 0x0Fu : axis == 1 ? 0x33u : 0x55u) << (up ? 4u >> axis : 0u);  // the children at that face
        if (!(vm & side)) continue;
        const uint64_t mask = morton_axis_mask(axis, levels);
        uint32_t there;
        if ((cell & mask) == (up ? mask : 0u)) {
            there = closed ? 0xFFu : 0u;  // the cell lies outside the grid (always, for the root group)
        } else {
            const uint64_t to = morton_step(cell, mask, up);
            // the levels that `to` shares with the first group's path
            const uint32_t d = min(levels, lead_levels);
            const uint64_t x = (to >> 3u * (levels - d)) ^ (lead_cell >> 3u * (lead_levels - d));
            uint32_t j = x ? d - 1u - (63u - (uint32_t)__clzll((long long)x)) / 3u : d;
            uint32_t group = path[wave][j];
            for (;; j++) {
                if (j == levels) {  // the neighbour is a group of this level
                    there = solid_mask(*reinterpret_cast<const uint4 *>(words + group), *reinterpret_cast<const uint4 *>(words + group + 4));
                    break;
                }
                const uint32_t p = words[group + (uint32_t(to >> 3u * (levels - 1u - j)) & 7u)] >> 4;
                if (p >= SVO_VOXEL_OFFSET) {  // a coarser voxel covers all four faces, the empty word none
                    there = p > SVO_VOXEL_OFFSET ? 0xFFu : 0u;
                    break;
                }
                group = p;
            }
        }
        beside |= uint64_t(there) << 8u * f;
    }

    uint32_t rank = start[k], child = first_child[k];
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        if (pointer[c] > SVO_VOXEL_OFFSET) {
            uint32_t faces = 0;
#pragma unroll
            for (uint32_t f = 0; f < 6; f++) {
                const uint32_t bit = 4u >> (f >> 1), other = c ^ bit;
                const bool outer = ((c & bit) != 0u) == ((f & 1u) != 0u);
                const uint32_t covered = outer ? uint32_t(beside >> (8u * f + other)) : vm >> other;
                faces |= (~covered & 1u) << f;
            }
            if (rank < n_list) {  // (always: n_list is the root's count)
                ent_key[rank] = prefix << 3 | c;
                ent_value[rank] = pointer[c] - SVO_VOXEL_OFFSET;
                ent_mask[rank] = uint8_t(faces);
            }
            rank++;
        } else if (pointer[c] < SVO_VOXEL_OFFSET) {
            if (vm >> (c + 1u)) rank += uint32_t(cnt[child]);  // (a voxel follows: the entries below this word lie before it)
            child++;
        }
    }
}

// The compaction's items: the list's mask bytes, 16 per thread in one uint4; a byte behind the list is 0.
struct Faces {
    const uint8_t *mask;  // room for a multiple of 16 bytes
    uint32_t mode;
    __device__ uint4 load(uint32_t i0, uint32_t m) const {
        if (i0 >= m) return uint4{0u, 0u, 0u, 0u};
        const uint4 s = *reinterpret_cast<const uint4 *>(mask + i0);
        uint32_t v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t left = m - i0 > 4u * q ? m - i0 - 4u * q : 0u;  // live bytes of this word
            const uint32_t live = left >= 4u ? 0xFFFFFFFFu : (1u << 8u * left) - 1u;
            v[q] = (v[q] | (mode == kModeAll ? kKept * 0x01010101u : 0u)) & live;
        }
        return uint4{v[0], v[1], v[2], v[3]};
    }
    __device__ uint32_t count(const uint4 &s) const {
        const uint32_t v[4] = {s.x, s.y, s.z, s.w};
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t b = (v[j >> 2] >> 8u * (j & 3u)) & 0xFFu;
            sum += mode == kModeQuads ? __popc(b) : b ? 1u : 0u;
        }
        return sum;
    }
};

struct FacesOut {
    const uint64_t *ent_key;
    const uint32_t *ent_value;
    uint32_t depth, n;              // n: the entries of the output
    uint32_t *xyz, *value, *level, *face;  // level may be null
    __device__ void write(uint32_t at, uint32_t x, uint32_t y, uint32_t z, uint32_t v, uint32_t l, uint32_t f) const {
        if (at >= n) return;  // (never: n is the scan's total)
        xyz[3ull * at] = x;
        xyz[3ull * at + 1] = y;
        xyz[3ull * at + 2] = z;
        value[at] = v;
        if (level) level[at] = l;
        face[at] = f;
    }
    __device__ void operator()(const Faces &items, uint32_t i0, const uint4 &s, uint32_t rank) const {
        const uint32_t v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t b = (v[j >> 2] >> 8u * (j & 3u)) & 0xFFu;
            if (!b) continue;
            const uint64_t cell = ent_key[i0 + j];
            const uint32_t l = key_bits(cell), val = ent_value[i0 + j];
            uint32_t x, y, z;
            morton_decode<uint64_t>(cell ^ (1ull << 3u * l), l, x, y, z);
            x <<= depth - l, y <<= depth - l, z <<= depth - l;
            if (items.mode == kModeQuads) {
                for (uint32_t f = 0; f < 6; f++)
                    if (b >> f & 1u) write(rank++, x, y, z, val, l, f);
            } else {
                write(rank++, x, y, z, val, l, b & 0x3Fu);
            }
        }
    }
};

enum Ev { kEvStart, kEvDiscover, kEvCount, kEvOffsets, kEvMask, kEvScan, kEvEmit, kEvs };

}  // namespace

// Per-context workspace of the surface pass (svo_ctx::surface): a listing plan of its own, 13 bytes per list entry, the
// tile sums; in the merge's instance (svo_surface_list_quads) the quads too, 24 bytes each.
struct svo_surface_state {
    svo_list_plan plan;
    svo_dev<uint64_t> ent_key;
    svo_dev<uint32_t> ent_value;
    svo_dev<uint8_t> ent_mask;
    svo_dev<uint32_t> tile_sum;
    svo_dev<uint32_t> quad_xyz, quad_value, quad_level, quad_face;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_SURFACE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        if (int rc = plan.create(ctx)) return rc;
        return status.alloc(ctx, kStWords);
    }
};

namespace {

// The pass behind its argument checks, in the workspace `slot`: into the caller's outputs, or, with `own`, the quads into
// the workspace's own arrays, whatever their number.
int list_surface(svo_ctx *ctx, svo_workspace<svo_surface_state> &slot, const svo_surface_params *p, uint32_t *xyz_out_dev,
                 uint32_t *value_out_dev, uint32_t *level_out_dev, uint32_t *face_out_dev, uint64_t *n_out, svo_surface_quads *own) {
    int rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), depth = p->depth;
    const uint32_t mode = p->flags & SVO_SURFACE_QUADS ? kModeQuads : p->flags & SVO_SURFACE_KEEP_HIDDEN ? kModeAll : kModeSurface;
    if ((rc = svo_workspace_ensure(ctx, slot))) return rc;
    svo_surface_state *s = slot.get();
    if ((rc = s->plan.grow(ctx, n_words / 8)) || (rc = s->timer.begin(ctx))) return rc;

    // the passes read the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    if ((rc = svo_list_plan_count(ctx, &s->plan, p->n_words, depth, false, s->timer.ev[kEvDiscover]))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvCount));
    const svo_list_plan &pl = s->plan;
    const uint32_t n_list = (uint32_t)pl.count, n_tiles = svo_div_up(n_list, kTile);  // (below 2^31: the plan refused more)
    uint64_t total = 0;
    if (n_list) {
        if ((rc = svo_grow(ctx, size_t(n_tiles) * kTile, &s->ent_key, &s->ent_value, &s->ent_mask)) ||
            (rc = svo_grow(ctx, (size_t)n_tiles, &s->tile_sum)))
            return rc;
        if ((rc = svo_list_plan_offsets(ctx, &s->plan, depth, false))) return rc;
        HIP_TRY(ctx, s->timer.mark(ctx, kEvOffsets));

        const uint32_t m = pl.walk.level_off[pl.listed];
        surface_mask_kernel<<<svo_div_up(m, kThreads), kThreads, 0, ctx->stream>>>(
            ctx->nodes, pl.walk.order, m, pl.walk.first_child, pl.cnt, pl.start, pl.key, p->flags & SVO_SURFACE_CLOSED_BOUNDARY ? 1u : 0u, n_list,
            s->ent_key, s->ent_value, s->ent_mask);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, s->timer.mark(ctx, kEvMask));

        const Faces live{s->ent_mask, mode};
        if ((rc = svo_tile_count(ctx, live, n_tiles, nullptr, n_list, s->tile_sum, s->status.dev + kStTotal))) return rc;
        if ((rc = s->status.read(ctx))) return rc;
        total = s->status.host()[kStTotal];  // (at most 6 per entry: no wrap)
    } else {
        HIP_TRY(ctx, s->timer.mark(ctx, kEvOffsets));
        HIP_TRY(ctx, s->timer.mark(ctx, kEvMask));
    }
    if (total >= kMaxEntries) return svo_fail(ctx, SVO_ERR_CAP, "the list has " + std::to_string(total) + " entries, 2^31 or more");
    if (xyz_out_dev && !own && total > p->max_entries)
        return svo_fail(ctx, SVO_ERR_CAP, "the list has " + std::to_string(total) + " entries, more than max_entries = " +
                                              std::to_string(p->max_entries));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvScan));

    if (own) {
        if ((rc = svo_grow(ctx, 3 * (size_t)total, &s->quad_xyz)) || (rc = svo_grow(ctx, (size_t)total, &s->quad_value, &s->quad_level, &s->quad_face)))
            return rc;
        xyz_out_dev = s->quad_xyz, value_out_dev = s->quad_value, level_out_dev = s->quad_level, face_out_dev = s->quad_face;
        *own = svo_surface_quads{xyz_out_dev, value_out_dev, level_out_dev, face_out_dev, (uint32_t)total};
    }
    if (xyz_out_dev && total) {
        const Faces live{s->ent_mask, mode};
        const FacesOut out{s->ent_key, s->ent_value, depth, (uint32_t)total, xyz_out_dev, value_out_dev, level_out_dev, face_out_dev};
        tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(live, out, nullptr, n_list, s->tile_sum);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEmit));
    if (n_out) *n_out = total;
    s->timer.finish(t0);
    return SVO_OK;
}

}  // namespace

// The exposed faces as SVO_SURFACE_QUADS lists them, for the merge (svo_surface_merge.hip), which has checked the arguments.
int svo_surface_list_quads(svo_ctx *ctx, svo_workspace<svo_surface_state> &slot, uint32_t closed_boundary, uint32_t depth,
                           uint64_t n_words, svo_surface_quads *out) {
    const svo_surface_params p{SVO_SURFACE_QUADS | (closed_boundary ? SVO_SURFACE_CLOSED_BOUNDARY : 0u), depth, n_words, 0};
    return list_surface(ctx, slot, &p, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}

extern "C" {

int svo_nodes_list_surface(svo_ctx *ctx, const svo_surface_params *p, uint32_t *xyz_out_dev, uint32_t *value_out_dev,
                           uint32_t *level_out_dev, uint32_t *face_out_dev, uint64_t *n_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    const uint32_t known = SVO_SURFACE_CLOSED_BOUNDARY | SVO_SURFACE_KEEP_HIDDEN | SVO_SURFACE_QUADS;
    if ((p->flags & ~known) || ((p->flags & SVO_SURFACE_QUADS) && (p->flags & SVO_SURFACE_KEEP_HIDDEN)))
        return svo_fail(ctx, SVO_ERR_ARG, "unknown or incompatible flag bits " + std::to_string(p->flags));
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (xyz_out_dev && (!value_out_dev || !face_out_dev))
        return svo_fail(ctx, SVO_ERR_ARG, "null face_out_dev or value_out_dev with xyz_out_dev given");
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, p->n_words))) return rc;
    return list_surface(ctx, ctx->surface, p, xyz_out_dev, value_out_dev, level_out_dev, face_out_dev, n_out, nullptr);
}

int svo_surface_timing(svo_ctx *ctx, float ms_out[SVO_SURFACE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->surface) return svo_fail(ctx, SVO_ERR_STATE, "no surface listed on this context yet");
    return ctx->surface->timer.read(ctx, ms_out);
}

}  // extern "C"

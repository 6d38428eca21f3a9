// svo_structure.hip -- voxel structures scattered over the tree in the node buffer: the highest occupied
// cell of every column of a rectangle (svo_nodes_column_tops), the columns that get a structure (svo_structures_sites)
// and the voxel list of a structure stamped at every site (svo_structures_stamp), which svo_nodes_edit takes.  The first
// only reads the words, enqueues one kernel and returns; the other two need no tree, count with one scan, block once to
// read the count and enqueue the fill.  No atomics anywhere: every output depends on its inputs alone.
//
//   tops     one lane per column, z fastest across lanes as in the output.  The lane walks down to the cell (x, y, z) from
//            y = y_hi - 1; an empty word met at level l clears its whole cube, so the search goes on below the cube, at
//            y = (y >> (depth - l) << (depth - l)) - 1, and the work follows the words on the column's way down, not its
//            2^depth cells.  The groups on the lane's path are kept in LDS as [level][lane] (a lane's bank is its number,
//            whatever its level), so the walk to the next cell starts at the deepest group the two cells share: the level
//            of the highest bit in which their y differ.  A coloured leaf, an interior word at `depth` (FINER) or a pointer
//            that fails svo_nodes_sample's check (BROKEN) ends the column; no pointer is followed before that check, and
//            every step either goes one level down, `depth` at the most, or moves y down
//   sites    a tile pass of svo_scan.h over the columns (count, scan, emit), with "the column is a site" as the flag
//   stamp    the entries (placement p, voxel v) are numbered p * m + v, which is the contract's order.  A check kernel
//            finds the lowest placement and voxel whose numbers are out of range (block minima, then one block over them).
//            Then a tile pass over the entries with the entry inside the grid as the flag, its emit the row-wise one
//            (tile_scatter_kernel).  Every entry is tested, also those of a placement that lies wholly inside the grid
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_morton.h"  // (morton_child)
#include "svo_scan.h"    // (kThreads, kPer, kTile, block_min, min_of_blocks_kernel, the tile pass)

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;
constexpr uint32_t kMaxDepth = 21;
constexpr uint32_t kNoBad = 0xFFFFFFFFu;
constexpr uint32_t kReach = 1u << 22;  // origins lie in [-kReach, kReach), offsets in (-kReach, kReach)
// the words read back: the scan's total; the lowest placement with a bad origin, with a bad rotation, the lowest voxel
// with a bad offset
enum Status { kStTotal, kStBadOrigin, kStBadRot, kStBadOffset, kStWords };

struct Columns {
    uint32_t ox, oz, sz;  // the rectangle's origin, its size along z
    uint32_t n;           // columns
};

// One lane per column (see the file's head).  stack[l - 1][lane] is the group of level l on the lane's path.
__global__ __launch_bounds__(kThreads) void column_tops_kernel(const uint32_t *__restrict__ words, uint64_t n_words, uint32_t depth,
                                                               uint32_t y_lo, uint32_t y_hi, Columns c, uint32_t *__restrict__ top_out,
                                                               uint32_t *__restrict__ value_out) {
    __shared__ uint32_t stack[kMaxDepth][kThreads];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kThreads + t;
    if (i >= c.n) return;
    const uint32_t x = c.ox + i / c.sz, z = c.oz + i % c.sz;
    uint32_t y = y_hi - 1u, level = 1, group = 0, top = SVO_TOP_NONE, value = 0;
    stack[0][t] = 0u;
    for (;;) {
        const uint32_t pointer = words[group + morton_child(x, y, z, depth - level)] >> 4;
        if (pointer >= SVO_VOXEL_OFFSET) {
            if (pointer != SVO_VOXEL_OFFSET) {
                top = y;
                value = pointer - SVO_VOXEL_OFFSET;
                break;
            }
            // an empty cube of level `level`: on below it
            const uint32_t shift = depth - level, floor = y >> shift << shift;
            if (floor <= y_lo) break;
            const uint32_t next = floor - 1u;
            level = depth - (31u - (uint32_t)__clz(int(y ^ next)));  // (next differs from y in a bit >= shift: no deeper than before)
            group = stack[level - 1u][t];
            y = next;
            continue;
        }
        if (level >= depth) {
            top = y;
            value = SVO_SAMPLE_FINER;
            break;
        }
        if ((pointer & 7u) || uint64_t(pointer) + 8u > n_words) {
            top = y;
            value = SVO_SAMPLE_BROKEN;
            break;
        }
        group = pointer;
        stack[level++][t] = group;
    }
    top_out[i] = top;
    if (value_out) value_out[i] = value;
}

__device__ inline uint32_t lowbias32(uint32_t v) {
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return v;
}

struct Sites {
    const uint32_t *top, *value;  // value may be null
    Columns c;
    uint32_t seed, one_in, on_value, rotate;
    int32_t lift;

    // whether column i is a site; its coordinates, top and hash
    __device__ bool at(uint32_t i, uint32_t &x, uint32_t &z, uint32_t &t, uint32_t &h) const {
        if (i >= c.n) return false;
        t = top[i];
        if (t == SVO_TOP_NONE) return false;
        if (value) {
            const uint32_t v = value[i];
            if (v >= SVO_VOXEL_OFFSET || (on_value && v != on_value)) return false;
        }
        x = c.ox + i / c.sz;
        z = c.oz + i % c.sz;
        h = lowbias32(lowbias32(x + seed) ^ z);
        return h % one_in == 0u;
    }
    // the tile pass's items (svo_scan.h): the state is the mask of a thread's columns that are sites
    __device__ uint32_t load(uint32_t i0, uint32_t) const {
        uint32_t mask = 0, x, z, t, h;
        for (uint32_t k = 0; k < kPer; k++) mask |= at(i0 + k, x, z, t, h) ? 1u << k : 0u;
        return mask;
    }
    __device__ uint32_t count(uint32_t mask) const { return __popc(mask); }
};

struct SitesOut {
    uint32_t room;
    int32_t *origins;
    uint32_t *rots;  // or null
    __device__ void operator()(const Sites &s, uint32_t i0, uint32_t mask, uint32_t o) const {
        for (uint32_t x, z, top, h; mask; mask &= mask - 1u, o++) {
            if (o >= room) break;  // (never: room is the scan's total)
            s.at(i0 + __ffs(mask) - 1u, x, z, top, h);
            origins[3ull * o] = int32_t(x);
            origins[3ull * o + 1] = int32_t(top + uint32_t(s.lift));
            origins[3ull * o + 2] = int32_t(z);
            if (rots) rots[o] = s.rotate ? lowbias32(h + 0x9E3779B9u) >> 30 : 0u;
        }
    }
};

struct Stamp {
    const int32_t *offsets, *origins;
    const uint32_t *colours, *rots;  // rots may be null
    uint32_t m, k, n;                // voxels, placements, entries = k * m
    uint32_t depth;

    // The cell of entry (p, v), in wrapping arithmetic: what the check kernel refuses never gets to the outputs.
    __device__ bool cell(uint32_t p, uint32_t v, uint32_t &cx, uint32_t &cy, uint32_t &cz) const {
        const uint32_t dx = uint32_t(offsets[3ull * v]), dy = uint32_t(offsets[3ull * v + 1]), dz = uint32_t(offsets[3ull * v + 2]);
        const uint32_t r = rots ? rots[p] & 3u : 0u;
        // R (dx, dy, dz) = (dz, dy, -dx), r times
        const uint32_t rx = r == 0 ? dx : r == 1 ? dz : r == 2 ? 0u - dx : 0u - dz;
        const uint32_t rz = r == 0 ? dz : r == 1 ? 0u - dx : r == 2 ? 0u - dz : dx;
        cx = uint32_t(origins[3ull * p]) + rx;
        cy = uint32_t(origins[3ull * p + 1]) + dy;
        cz = uint32_t(origins[3ull * p + 2]) + rz;
        return ((cx | cy | cz) >> depth) == 0u;
    }
    // the tile pass's items (svo_scan.h): the state is the mask of a thread's entries that lie inside the grid
    __device__ uint32_t load(uint32_t i0, uint32_t) const {
        uint32_t mask = 0, cx, cy, cz;
        if (i0 >= n) return 0u;
        uint32_t p = i0 / m, v = i0 % m;
        for (uint32_t j = 0; j < kPer && i0 + j < n; j++) {
            mask |= cell(p, v, cx, cy, cz) ? 1u << j : 0u;
            if (++v == m) v = 0u, p++;
        }
        return mask;
    }
    __device__ uint32_t count(uint32_t mask) const { return __popc(mask); }
    __device__ uint32_t flags(uint32_t mask, uint32_t j) const { return mask >> j & 1u; }
};

struct StampOut {
    uint32_t room;
    uint32_t *xyz, *colour, *placement;  // placement may be null
    __device__ void operator()(const Stamp &s, uint32_t i, uint32_t, uint32_t o) const {
        if (o >= room) return;  // (never: room is the scan's total)
        const uint32_t p = i / s.m, v = i % s.m;
        uint32_t cx, cy, cz;
        s.cell(p, v, cx, cy, cz);
        const uint32_t c = s.colours[v];  // (with the cell's loads, not behind the stores that may alias it)
        xyz[3ull * o] = cx;
        xyz[3ull * o + 1] = cy;
        xyz[3ull * o + 2] = cz;
        colour[o] = c;
        if (placement) placement[o] = p;
    }
};

// One lane per placement and per voxel: block_bad[3 * block + {0, 1, 2}] the block's lowest placement with a bad origin,
// with a bad rotation, its lowest voxel with a bad offset.
__global__ __launch_bounds__(kThreads) void stamp_check_kernel(Stamp s, uint32_t *__restrict__ block_bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t bad_origin = kNoBad, bad_rot = kNoBad, bad_offset = kNoBad;
    if (i < s.k) {
        for (uint32_t a = 0; a < 3; a++)
            if (uint32_t(s.origins[3ull * i + a]) + kReach >= 2u * kReach) bad_origin = i;
        if (s.rots && s.rots[i] >= 4u) bad_rot = i;
    }
    if (i < s.m)
        for (uint32_t a = 0; a < 3; a++)
            if (uint32_t(s.offsets[3ull * i + a]) + (kReach - 1u) >= 2u * kReach - 1u) bad_offset = i;
    bad_origin = block_min<kThreads>(bad_origin);
    bad_rot = block_min<kThreads>(bad_rot);
    bad_offset = block_min<kThreads>(bad_offset);
    if (threadIdx.x == 0) {
        block_bad[3ull * blockIdx.x] = bad_origin;
        block_bad[3ull * blockIdx.x + 1] = bad_rot;
        block_bad[3ull * blockIdx.x + 2] = bad_offset;
    }
}

enum Ev { kEvStart, kEvCount, kEvFill, kEvs };

}  // namespace

// Per-context workspace of the three calls (svo_ctx::structure): one u32 per tile of columns or entries, three per
// block of the stamp's check.
struct svo_structure_state {
    svo_dev<uint32_t> tiles, bad;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_STRUCTURE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
    // the fill's span: empty (0 ms) for a call that fills nothing, else from the count's event to the one recorded here
    void no_fill() { timer.span[1][0] = timer.span[1][1] = timer.ev[kEvCount]; }
    hipError_t fill_done(svo_ctx *ctx) {
        timer.span[1][1] = timer.ev[kEvFill];
        return timer.mark(ctx, kEvFill);
    }
};

namespace {

// origin + size of a rectangle on the x-z plane and its columns; the pointers are the caller's to check
uint64_t columns_of(const uint32_t origin_xz[2], const uint32_t size_xz[2], Columns *c) {
    *c = Columns{origin_xz[0], origin_xz[1], size_xz[1], 0u};
    return uint64_t(size_xz[0]) * size_xz[1];
}

std::string cap_message(const char *what, uint64_t count, const char *room_name, uint64_t room) {
    return std::string("the list has ") + std::to_string(count) + " " + what + ", more than " + room_name + " = " + std::to_string(room);
}

}  // namespace

extern "C" {

int svo_nodes_column_tops(svo_ctx *ctx, const svo_tops_params *p, const uint32_t origin_xz[2], const uint32_t size_xz[2],
                          uint32_t *top_out_dev, uint32_t *value_out_dev) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!origin_xz) return svo_fail(ctx, SVO_ERR_ARG, "null origin_xz");
    if (!size_xz) return svo_fail(ctx, SVO_ERR_ARG, "null size_xz");
    if (!top_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null top_out_dev");
    int rc = svo_check_flags(ctx, p->flags, 0);
    if (rc || (rc = svo_check_depth(ctx, p->depth, kMaxDepth))) return rc;
    const uint64_t side = 1ull << p->depth;
    if (p->y_lo >= p->y_hi || p->y_hi > side)
        return svo_fail(ctx, SVO_ERR_ARG, "the y range must be y_lo < y_hi <= 2^depth = " + std::to_string(side) + " (got " +
                                              std::to_string(p->y_lo) + ", " + std::to_string(p->y_hi) + ")");
    for (int a = 0; a < 2; a++)
        if (uint64_t(origin_xz[a]) + size_xz[a] > side)
            return svo_fail(ctx, SVO_ERR_ARG, std::string("the rectangle leaves the grid on ") + (a ? "z" : "x") + ": origin " +
                                                  std::to_string(origin_xz[a]) + " + size " + std::to_string(size_xz[a]) +
                                                  " > 2^depth = " + std::to_string(side));
    Columns c;
    const uint64_t columns = columns_of(origin_xz, size_xz, &c);  // (each size at most 2^21: no wrap)
    if (columns >= kMaxEntries) return svo_fail(ctx, SVO_ERR_ARG, "the rectangle has " + std::to_string(columns) + " columns, 2^31 or more");
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, p->n_words))) return rc;
    if (!columns) return SVO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    if ((rc = svo_workspace_ensure(ctx, ctx->structure))) return rc;
    svo_structure_state *s = ctx->structure.get();
    c.n = (uint32_t)columns;
    // the kernel reads the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    column_tops_kernel<<<svo_div_up(columns, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, p->n_words, p->depth, p->y_lo, p->y_hi, c,
                                                                                  top_out_dev, value_out_dev);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvCount));
    s->no_fill();
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_structures_sites(svo_ctx *ctx, const svo_sites_params *p, const uint32_t *top_dev, const uint32_t *value_dev,
                         const uint32_t origin_xz[2], const uint32_t size_xz[2], int32_t *origins_out_dev, uint32_t *rots_out_dev,
                         uint64_t *n_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    int rc = svo_check_flags(ctx, p->flags, SVO_SITES_ROTATE);
    if (rc) return rc;
    if (!p->one_in) return svo_fail(ctx, SVO_ERR_ARG, "one_in must be at least 1");
    if (!origin_xz) return svo_fail(ctx, SVO_ERR_ARG, "null origin_xz");
    if (!size_xz) return svo_fail(ctx, SVO_ERR_ARG, "null size_xz");
    for (int a = 0; a < 2; a++)
        if (origin_xz[a] >= kMaxEntries || size_xz[a] >= kMaxEntries)
            return svo_fail(ctx, SVO_ERR_ARG, std::string("origin and size must be below 2^31 on ") + (a ? "z" : "x") + " (got " +
                                                  std::to_string(origin_xz[a]) + ", " + std::to_string(size_xz[a]) + ")");
    Columns c;
    const uint64_t columns = columns_of(origin_xz, size_xz, &c);  // (each size below 2^31: no wrap)
    if (columns >= kMaxEntries) return svo_fail(ctx, SVO_ERR_ARG, "the rectangle has " + std::to_string(columns) + " columns, 2^31 or more");
    if (columns && !top_dev) return svo_fail(ctx, SVO_ERR_ARG, "null top_dev");
    if (p->on_value && !value_dev) return svo_fail(ctx, SVO_ERR_ARG, "null value_dev with on_value given");
    if (!columns) {
        *n_out = 0;
        return SVO_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    if ((rc = svo_workspace_ensure(ctx, ctx->structure))) return rc;
    svo_structure_state *s = ctx->structure.get();
    if ((rc = s->timer.begin(ctx))) return rc;
    c.n = (uint32_t)columns;
    const Sites sites{top_dev, value_dev, c, p->seed, p->one_in, p->on_value, p->flags & SVO_SITES_ROTATE, p->lift};
    const uint32_t n_tiles = svo_div_up(columns, kTile);
    if ((rc = svo_grow(ctx, (size_t)n_tiles, &s->tiles))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    if ((rc = svo_tile_count(ctx, sites, n_tiles, nullptr, c.n, s->tiles, s->status.dev + kStTotal))) return rc;
    if ((rc = s->status.read(ctx))) return rc;
    const uint64_t count = s->status.host()[kStTotal];
    if (origins_out_dev && count > p->max_sites) return svo_fail(ctx, SVO_ERR_CAP, cap_message("sites", count, "max_sites", p->max_sites));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvCount));
    s->no_fill();
    if (origins_out_dev && count) {
        tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(sites, SitesOut{(uint32_t)count, origins_out_dev, rots_out_dev}, nullptr, c.n, s->tiles);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, s->fill_done(ctx));
    }
    *n_out = count;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_structures_stamp(svo_ctx *ctx, const svo_stamp_params *p, const int32_t *offsets_dev, const uint32_t *colours_dev, size_t m,
                         const int32_t *origins_dev, const uint32_t *rots_dev, size_t k, uint32_t *xyz_out_dev, uint32_t *colour_out_dev,
                         uint32_t *placement_out_dev, uint64_t *n_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    int rc = svo_check_flags(ctx, p->flags, 0);
    if (rc || (rc = svo_check_depth(ctx, p->depth, kMaxDepth))) return rc;
    if (k >= kMaxEntries || m >= kMaxEntries || uint64_t(k) * m >= kMaxEntries)
        return svo_fail(ctx, SVO_ERR_ARG, std::to_string(k) + " placements of " + std::to_string(m) + " voxels are 2^31 entries or more");
    const uint64_t entries = uint64_t(k) * m;
    if (entries && !offsets_dev) return svo_fail(ctx, SVO_ERR_ARG, "null offsets_dev");
    if (entries && !colours_dev) return svo_fail(ctx, SVO_ERR_ARG, "null colours_dev");
    if (entries && !origins_dev) return svo_fail(ctx, SVO_ERR_ARG, "null origins_dev");
    if (xyz_out_dev && !colour_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null colour_out_dev with xyz_out_dev given");
    if (!entries) {
        *n_out = 0;
        return SVO_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    if ((rc = svo_workspace_ensure(ctx, ctx->structure))) return rc;
    svo_structure_state *s = ctx->structure.get();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t *st = s->status.host();
    const Stamp stamp{offsets_dev, origins_dev, colours_dev, rots_dev, (uint32_t)m, (uint32_t)k, (uint32_t)entries, p->depth};
    const uint32_t n_tiles = svo_div_up(entries, kTile), n_check = svo_div_up(std::max(k, m), kThreads);
    if ((rc = svo_grow(ctx, (size_t)n_tiles, &s->tiles)) || (rc = svo_grow(ctx, 3 * (size_t)n_check, &s->bad))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    stamp_check_kernel<<<n_check, kThreads, 0, ctx->stream>>>(stamp, s->bad);
    min_of_blocks_kernel<3><<<1, kTopThreads, 0, ctx->stream>>>(s->bad, n_check, s->status.dev + kStBadOrigin);
    if ((rc = svo_tile_count(ctx, stamp, n_tiles, nullptr, stamp.n, s->tiles, s->status.dev + kStTotal))) return rc;
    if ((rc = s->status.read(ctx))) return rc;
    if (st[kStBadOrigin] != kNoBad)
        return svo_fail(ctx, SVO_ERR_ARG, "placement " + std::to_string(st[kStBadOrigin]) + " has an origin component outside [-2^22, 2^22)");
    if (st[kStBadRot] != kNoBad)
        return svo_fail(ctx, SVO_ERR_ARG, "placement " + std::to_string(st[kStBadRot]) + " has a rotation outside 0..3");
    if (st[kStBadOffset] != kNoBad)
        return svo_fail(ctx, SVO_ERR_ARG, "voxel " + std::to_string(st[kStBadOffset]) + " has an offset component outside (-2^22, 2^22)");
    const uint64_t count = st[kStTotal];
    if (xyz_out_dev && count > p->max_voxels) return svo_fail(ctx, SVO_ERR_CAP, cap_message("entries", count, "max_voxels", p->max_voxels));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvCount));
    s->no_fill();
    if (xyz_out_dev && count) {
        tile_scatter_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(stamp, StampOut{(uint32_t)count, xyz_out_dev, colour_out_dev, placement_out_dev},
                                                                   stamp.n, s->tiles);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, s->fill_done(ctx));
    }
    *n_out = count;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_structure_timing(svo_ctx *ctx, float ms_out[SVO_STRUCTURE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->structure) return svo_fail(ctx, SVO_ERR_STATE, "no structure call has run on this context yet");
    return ctx->structure->timer.read(ctx, ms_out);
}

}  // extern "C"

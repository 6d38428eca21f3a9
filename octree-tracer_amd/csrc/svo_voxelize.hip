// svo_voxelize.hip -- triangle meshes voxelised on the device: one entry per (triangle, cell of the
// `depth` grid) whose closed triangle meets the closed cube, in ascending triangle index and, within a triangle, in
// ascending Morton order of the cell.  The pairs are refined breadth-first, one level at a time, from one pair per
// triangle at the root; no sort and no atomics, so the list is the same on every run.  One lane per pair.
//
//   setup    one lane per triangle: the vertex indices and coordinates are checked, the nine doubled coordinates 2q + 1
//            gathered into the workspace (no later kernel follows an index of the caller's), the root pair written; the
//            first bad triangle is the minimum over the blocks' minima
//   test     per level, one lane per pair: the 8-bit mask of the children that the triangle meets.  A triangle whose
//            bounding box lies in one cell of the level is inside that cell, which is a child of the pair's: a shift and
//            a compare.  Otherwise the 13 separating axes, with everything that does not depend on the child (edges,
//            normal, the plane's and the edges' projections relative to the parent's centre) outside the 8-child loop
//   sum      a tile pass of svo_scan.h over the pairs' masks, whose set bits are counted; vox_total_kernel adds the
//            tiles' sums in 64 bits (8 children of up to 2^31 pairs do not fit 32) before tile_offsets_kernel scans
//            them; the total comes back to the host, which refuses a level over the cap before anything is allocated
//   scatter  the pass's row-wise emit (tile_scatter_kernel): each pair's children in child order behind the pair's
//            rank: the input order by triangle and the child order within a pair are the contract's order.  The last
//            level writes the caller's outputs instead of the next pair array
//
// The arithmetic is exact (include/svo_hip.h): doubled coordinates are odd and below 2^28, a cell's bounds even.  Edge
// tests fit int64 (terms below 2^58), the plane test takes 128-bit products.  No float anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "svo_ctx.h"
#include "svo_mesh.h"  // (the triangles' check and gather, shared with svo_solid.hip)
#include "svo_scan.h"  // (kThreads, kTile, block_min, min_of_blocks_kernel, the tile pass's kernels)

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;
constexpr uint32_t kNoBad = kNoBadTriangle;
// the words read back: the first bad triangle << 1 | (0: a vertex index, 1: a coordinate), the level's pair count in two halves
enum Status { kStBad, kStCountLo, kStCountHi, kStWords };

typedef __int128 i128;

// a cell's coordinates (21 bits each) in one word
__device__ inline uint64_t cell_pack(uint32_t x, uint32_t y, uint32_t z) { return uint64_t(x) << 42 | uint64_t(y) << 21 | z; }
__device__ inline uint32_t cell_x(uint64_t c) { return uint32_t(c >> 42); }
__device__ inline uint32_t cell_y(uint64_t c) { return uint32_t(c >> 21) & 0x1FFFFFu; }
__device__ inline uint32_t cell_z(uint64_t c) { return uint32_t(c) & 0x1FFFFFu; }

// One lane per triangle.  tv gets its doubled coordinates (of a bad triangle: those of q = 0, so that every later pass
// runs on it without harm until the host has read the verdict), the pair arrays the root pair.
__global__ __launch_bounds__(kThreads) void vox_setup_kernel(const uint32_t *__restrict__ vq, uint32_t n_vertices,
                                                             const uint32_t *__restrict__ tri, uint32_t n_tris, uint32_t depth,
                                                             int32_t *__restrict__ tv, uint32_t *__restrict__ pair_tri,
                                                             uint64_t *__restrict__ pair_cell, uint32_t *__restrict__ block_bad) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    uint32_t bad = kNoBad;
    if (t < n_tris) {
        int32_t v[9];
        bad = mesh_gather_triangle(vq, n_vertices, tri, t, depth, v);
        for (uint32_t k = 0; k < 9; k++) tv[9ull * t + k] = v[k];
        pair_tri[t] = t;
        pair_cell[t] = 0;
    }
    bad = block_min<kThreads>(bad);
    if (threadIdx.x == 0) block_bad[blockIdx.x] = bad;
}

__device__ inline int64_t abs64(int64_t v) { return v < 0 ? -v : v; }
// v * 2^k (the products fit: see the file's head)
__device__ inline int64_t shl(int64_t v, uint32_t k) { return int64_t(uint64_t(v) << k); }
__device__ inline i128 shl(i128 v, uint32_t k) { return i128((unsigned __int128)v << k); }

// The children of the level-(l - 1) cell (px, py, pz) that the triangle v (nine doubled coordinates) meets, as a mask by
// child index x * 4 + y * 2 + z.  hs = depth - l + 6: a child's half side in doubled units is h = 2^hs.  The pair itself
// overlaps (the refinement's invariant).
__device__ inline uint32_t child_mask(const int32_t *__restrict__ v, uint32_t px, uint32_t py, uint32_t pz, uint32_t hs) {
    // the cheap path: the bounding box lies in one cell of level l
    uint32_t lo_cell[3], same = 1;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int32_t lo = min(v[a], min(v[3 + a], v[6 + a])), hi = max(v[a], max(v[3 + a], v[6 + a]));
        lo_cell[a] = uint32_t(lo) >> (hs + 1);
        same &= lo_cell[a] == uint32_t(hi) >> (hs + 1);
    }
    if (same) return 1u << ((lo_cell[0] & 1u) << 2 | (lo_cell[1] & 1u) << 1 | (lo_cell[2] & 1u));

    // everything relative to the parent's centre: a child's centre is at (sx, sy, sz) * h with s = +-1
    const uint32_t p[3] = {px, py, pz};
    const int32_t side = 1 << (hs + 1);  // a child's side
    int32_t w[3][3], e[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int32_t centre = int32_t((2u * p[a] + 1u) << (hs + 1));
#pragma unroll
        for (int j = 0; j < 3; j++) {
            w[j][a] = v[3 * j + a] - centre;
            e[j][a] = v[3 * ((j + 1) % 3) + a] - v[3 * j + a];
        }
    }
    // the box axes: per axis, whether the lower and the upper half meet the triangle's extent
    bool half_ok[3][2];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int32_t lo = min(w[0][a], min(w[1][a], w[2][a])), hi = max(w[0][a], max(w[1][a], w[2][a]));
        half_ok[a][0] = !(lo > 0 || hi < -side);
        half_ok[a][1] = !(lo > side || hi < 0);
    }
    // the plane: n . (w0 - s h) against h (|nx| + |ny| + |nz|)
    int64_t n[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        n[a] = int64_t(e[0][b]) * e[1][c] - int64_t(e[0][c]) * e[1][b];
    }
    const i128 plane = i128(n[0]) * w[0][0] + i128(n[1]) * w[0][1] + i128(n[2]) * w[0][2];
    const int64_t reach = abs64(n[0]) + abs64(n[1]) + abs64(n[2]);
    // the edge axes unit_a x e_i: the projection -e_c x_b + e_b x_c has one value on the edge's two vertices and one on the
    // third; lo and hi of the two, and the box's reach h (|e_b| + |e_c|)
    int64_t proj_lo[3][3], proj_hi[3][3], edge_reach[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3, k = (i + 2) % 3;
            const int64_t on = int64_t(e[i][b]) * w[i][c] - int64_t(e[i][c]) * w[i][b];
            const int64_t off = int64_t(e[i][b]) * w[k][c] - int64_t(e[i][c]) * w[k][b];
            proj_lo[i][a] = min(on, off);
            proj_hi[i][a] = max(on, off);
            edge_reach[i][a] = shl(abs64(e[i][b]) + abs64(e[i][c]), hs);
        }
    }
    uint32_t mask = 0;
#pragma unroll
    for (int child = 0; child < 8; child++) {
        const int s[3] = {child & 4 ? 1 : -1, child & 2 ? 1 : -1, child & 1 ? 1 : -1};
        bool ok = half_ok[0][child >> 2 & 1] && half_ok[1][child >> 1 & 1] && half_ok[2][child & 1];
        const int64_t ns = s[0] * n[0] + s[1] * n[1] + s[2] * n[2];
        ok = ok && !(plane > shl(i128(ns + reach), hs) || plane < shl(i128(ns - reach), hs));
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int b = (a + 1) % 3, c = (a + 2) % 3;
                const int64_t shift = shl(int64_t(e[i][b]) * s[c] - int64_t(e[i][c]) * s[b], hs);
                ok = ok && !(proj_lo[i][a] - shift > edge_reach[i][a] || proj_hi[i][a] - shift < -edge_reach[i][a]);
            }
        }
        mask |= ok ? 1u << child : 0u;
    }
    return mask;
}

__global__ __launch_bounds__(kThreads) void vox_test_kernel(const int32_t *__restrict__ tv, const uint32_t *__restrict__ pair_tri,
                                                            const uint64_t *__restrict__ pair_cell, uint32_t m, uint32_t hs,
                                                            uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const int32_t *src = tv + 9ull * pair_tri[i];
    int32_t v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = src[k];
    const uint64_t cell = pair_cell[i];
    mask[i] = uint8_t(child_mask(v, cell_x(cell), cell_y(cell), cell_z(cell), hs));
}

// The tile pass's items: a level's pairs with their child masks, one byte per pair (svo_scan.h: FlagBytes).
struct Pairs : FlagBytes {
    const uint32_t *tri;
    const uint64_t *cell;
};

// before tile_offsets_kernel, which scans the sums in place: their total in 64 bits
static_assert(kStCountHi == kStCountLo + 1, "block_total64 writes the two halves side by side");
__global__ __launch_bounds__(kTopThreads) void vox_total_kernel(const uint32_t *tile_sum, uint32_t n_tiles, uint32_t *status) {
    block_total64(tile_sum, n_tiles, status + kStCountLo);
}

struct VoxOut {
    uint32_t *pair_tri;   // the next level's pairs, or
    uint64_t *pair_cell;
    uint32_t *xyz, *colour, *tri;  // (kEmit) the caller's outputs; tri may be null
    const uint32_t *tri_colours;   // or null: default_colour
    uint32_t default_colour;
    uint32_t room;  // entries the outputs hold: the level's total, which the host has checked
};

// the children `bits` of pair i, in child order from output o on
template <bool kEmit>
struct Children {
    VoxOut out;
    __device__ void operator()(const Pairs &p, uint32_t i, uint32_t bits, uint32_t o) const {
        const uint32_t t = p.tri[i];
        const uint64_t cell = p.cell[i];
        const uint32_t x = cell_x(cell) << 1, y = cell_y(cell) << 1, z = cell_z(cell) << 1;
        uint32_t colour = 0;
        if (kEmit) colour = (out.tri_colours ? out.tri_colours[t] : out.default_colour) & 0xFFFFFFu;
        for (; bits; bits &= bits - 1u, o++) {
            const uint32_t child = __ffs(bits) - 1u;
            if (o >= out.room) break;  // (never: room is the scan's total)
            const uint32_t cx = x | (child >> 2), cy = y | (child >> 1 & 1u), cz = z | (child & 1u);
            if (kEmit) {
                out.xyz[3ull * o] = cx;
                out.xyz[3ull * o + 1] = cy;
                out.xyz[3ull * o + 2] = cz;
                out.colour[o] = colour;
                if (out.tri) out.tri[o] = t;
            } else {
                out.pair_tri[o] = t;
                out.pair_cell[o] = cell_pack(cx, cy, cz);
            }
        }
    }
};

enum Ev { kEvStart, kEvSetup, kEvRefine, kEvCount, kEvEmit, kEvs };

}  // namespace

// Per-context workspace of the voxeliser (svo_ctx::voxelize): nine i32 per triangle, two pair arrays of twelve bytes per
// pair that take turns, one mask byte per pair, one u32 per tile.
struct svo_voxelize_state {
    svo_dev<int32_t> tv;  // (i32: nine per triangle)
    svo_dev<uint32_t> pair_tri[2];
    svo_dev<uint64_t> pair_cell[2];
    svo_dev<uint8_t> mask;
    svo_dev<uint32_t> tiles;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_VOXELIZE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

extern "C" {

int svo_mesh_voxelize(svo_ctx *ctx, const svo_voxelize_params *p, const uint32_t *vq_dev, const uint32_t *tri_dev,
                      const uint32_t *tri_colours_dev, size_t n_tris, uint32_t *xyz_out_dev, uint32_t *colour_out_dev,
                      uint32_t *tri_out_dev, uint64_t *n_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    int rc = svo_check_flags(ctx, p->flags, 0);
    if (rc || (rc = svo_check_depth(ctx, p->depth, 21))) return rc;
    if (n_tris >= kMaxEntries) return svo_fail(ctx, SVO_ERR_ARG, "n_tris must be below 2^31 (got " + std::to_string(n_tris) + ")");
    if (n_tris && !vq_dev) return svo_fail(ctx, SVO_ERR_ARG, "null vq_dev");
    if (n_tris && !tri_dev) return svo_fail(ctx, SVO_ERR_ARG, "null tri_dev");
    if (xyz_out_dev && !colour_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null colour_out_dev with xyz_out_dev given");
    if (!n_tris) {
        *n_out = 0;
        return SVO_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t depth = p->depth, n = (uint32_t)n_tris;
    if ((rc = svo_workspace_ensure(ctx, ctx->voxelize))) return rc;
    svo_voxelize_state *s = ctx->voxelize.get();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t *st = s->status.host();
    const uint64_t cap = xyz_out_dev ? std::min<uint64_t>(p->max_voxels, kMaxEntries - 1) : kMaxEntries - 1;

    // setup: the check, the gather, the root pairs
    const uint32_t n_blocks = svo_div_up(n, kThreads);
    if ((rc = svo_grow(ctx, 9 * (size_t)n, &s->tv))) return rc;
    if ((rc = svo_grow(ctx, (size_t)n, &s->pair_tri[0], &s->pair_cell[0]))) return rc;
    if ((rc = svo_grow(ctx, (size_t)n_blocks, &s->tiles))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    vox_setup_kernel<<<n_blocks, kThreads, 0, ctx->stream>>>(vq_dev, p->n_vertices, tri_dev, n, depth, s->tv, s->pair_tri[0],
                                                             s->pair_cell[0], s->tiles);
    min_of_blocks_kernel<1><<<1, kTopThreads, 0, ctx->stream>>>(s->tiles, n_blocks, s->status.dev + kStBad);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvSetup));

    uint32_t m = n, cur = 0;  // the pairs of level l - 1: pair_*[cur][0, m)
    for (uint32_t l = 1; l <= depth; l++) {
        if (l == depth) HIP_TRY(ctx, s->timer.mark(ctx, kEvRefine));
        const uint32_t n_tiles = svo_div_up(m, kTile), hs = depth - l + SVO_VOX_SUBBITS;
        if ((rc = svo_grow(ctx, size_t(n_tiles) * kTile, &s->mask))) return rc;
        if ((rc = svo_grow(ctx, (size_t)n_tiles, &s->tiles))) return rc;
        const Pairs pairs{{s->mask}, s->pair_tri[cur], s->pair_cell[cur]};
        vox_test_kernel<<<svo_div_up(m, kThreads), kThreads, 0, ctx->stream>>>(s->tv, s->pair_tri[cur], s->pair_cell[cur], m, hs, s->mask);
        tile_count_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(pairs, nullptr, m, s->tiles);
        vox_total_kernel<<<1, kTopThreads, 0, ctx->stream>>>(s->tiles, n_tiles, s->status.dev);
        tile_offsets_kernel<<<1, kTopThreads, 0, ctx->stream>>>(s->tiles, n_tiles, nullptr, 0, nullptr);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = s->status.read(ctx))) return rc;
        if (l == 1 && st[kStBad] != kNoBad)
            return svo_fail(ctx, SVO_ERR_ARG, mesh_bad_triangle(st[kStBad], depth, p->n_vertices));
        const uint64_t count = uint64_t(st[kStCountHi]) << 32 | st[kStCountLo];
        if (count > cap)
            return svo_fail(ctx, SVO_ERR_CAP, "level " + std::to_string(l) + " has " + std::to_string(count) + " (triangle, cell) pairs, " +
                                                  (count >= kMaxEntries ? "2^31 or more"
                                                                        : "more than max_voxels = " + std::to_string(p->max_voxels)));
        VoxOut out{};
        out.room = (uint32_t)count;
        if (l < depth) {
            const uint32_t next = cur ^ 1u;
            if ((rc = svo_grow(ctx, (size_t)count, &s->pair_tri[next], &s->pair_cell[next]))) return rc;
            out.pair_tri = s->pair_tri[next];
            out.pair_cell = s->pair_cell[next];
            tile_scatter_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(pairs, Children<false>{out}, m, s->tiles);
            HIP_TRY(ctx, hipGetLastError());
            m = (uint32_t)count;
            cur = next;
            continue;
        }
        HIP_TRY(ctx, s->timer.mark(ctx, kEvCount));
        if (xyz_out_dev && count) {
            out.xyz = xyz_out_dev;
            out.colour = colour_out_dev;
            out.tri = tri_out_dev;
            out.tri_colours = tri_colours_dev;
            out.default_colour = p->default_colour;
            tile_scatter_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(pairs, Children<true>{out}, m, s->tiles);
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, s->timer.mark(ctx, kEvEmit));
        *n_out = count;
    }
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_voxelize_timing(svo_ctx *ctx, float ms_out[SVO_VOXELIZE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->voxelize) return svo_fail(ctx, SVO_ERR_STATE, "no mesh voxelised on this context yet");
    return ctx->voxelize->timer.read(ctx, ms_out);
}

}  // extern "C"

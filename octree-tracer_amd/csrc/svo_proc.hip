// svo_proc.hip -- the procedural world generator (the reference's third kernel: procedual.wgsl main + sdf, driven by
// procedural.rs Procedural::generate_chunk and world.rs World::generate_world), restated deterministically
// (DESIGN.md 11).  The reference inserts every solid cell into a shared tree with unsynchronised atomics, so its node
// order changes from run to run; here the tree is the canonical breadth-first form of the same shape, built by scans:
//
//   classify   one lane per cell, lanes in Morton order (a wave64 covers a 4x4x4 brick): sdf, "above" sdf for solid
//              cells, one class byte per cell; __ballot(solid) is the child masks of the brick's 8 parents
//   reduce     child masks level by level up to the root (a node is interior iff its mask is non-zero)
//   ranks      per level, an exclusive scan of the interior flags in Morton order (a tile pass of svo_scan.h): every
//              interior node's rank, hence its child group's index, and the exact node count, which is read back and
//              checked before anything is emitted
//   emit       one lane per interior parent: its 8-node group in the 8-byte <id>.bin layout
//   mips       (svo_world_generate only) block leaves take their block's top_mip, then svo_mip.h's pass bottom-up
//
// All work runs on the context's stream.  Sizes come from the count pass; there are no atomics and no retries.
// Shared with the tree builder: the tile pass (svo_scan.h), the Morton convention (svo_morton.h), the mip pass
// (svo_mip.h), svo_grow for the workspace and svo_world_writer for svo_world_generate's directory (svo_ctx.h; the writer
// itself is in svo_build.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_host.h"
#include "svo_mip.h"     // (the world path mips its chunks on the device, as svo_world_build does)
#include "svo_morton.h"  // (lanes walk the cells in Morton order)
#include "svo_scan.h"    // (a level's mask bytes are scanned in tiles of kTile)

namespace {

constexpr uint32_t kChunkOffset = SVO_CHUNK_OFFSET;
constexpr uint64_t kDefaultMaxNodes = 256000000ull;  // procedural.rs:4

// ---- sdf (procedual.wgsl:109-148 over common.wgsl:43-191), one IEEE f32 operation per step, in the order of
// DESIGN.md 11; compiled with -ffp-contract=off, so no step is fused ----
namespace sdf {

__device__ inline float step(float edge, float x) { return x >= edge ? 1.0f : 0.0f; }
__device__ inline float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ inline float sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ inline float smoothstep(float e0, float e1, float x) {
    const float t = clamp01((x - e0) / (e1 - e0));
    return (t * t) * (3.0f - 2.0f * t);
}
// x % 289 (fmodf).  Every x this is called with is integer-valued: lattice coordinates are floor()s, and permute's
// arguments stay integers below 2^24 in magnitude (|x| < 579, so (x * 34 + 1) * x < 1.2e7 is exact).  For such x
// the integer remainder is the exact fmodf value (sign of the dividend; a zero's sign is lost, which the next
// `p - 49 * floor(...)` erases anyway) and costs a few instructions instead of fmodf's software loop.  Anything
// else (|x| >= 2^24, inf, NaN) takes fmodf itself.
__device__ inline float mod289(float x) {
    if (fabsf(x) < 16777216.0f) return float(int(x) % 289);
    return fmodf(x, 289.0f);
}
__device__ inline float permute(float x) { return mod289((x * 34.0f + 1.0f) * x); }

__device__ float simplex(float vx, float vy, float vz) {
    const float c6 = 1.0f / 6.0f, c3 = 1.0f / 3.0f;
    const float s = (vx * c3 + vy * c3) + vz * c3;
    float ix = floorf(vx + s), iy = floorf(vy + s), iz = floorf(vz + s);
    const float t = (ix * c6 + iy * c6) + iz * c6;
    float x0[3] = {(vx - ix) + t, (vy - iy) + t, (vz - iz) + t};
    const float g[3] = {step(x0[1], x0[0]), step(x0[2], x0[1]), step(x0[0], x0[2])};
    const float l[3] = {1.0f - g[0], 1.0f - g[1], 1.0f - g[2]};
    const float i1[3] = {fminf(g[0], l[2]), fminf(g[1], l[0]), fminf(g[2], l[1])};
    const float i2[3] = {fmaxf(g[0], l[2]), fmaxf(g[1], l[0]), fmaxf(g[2], l[1])};
    const float c6x2 = 2.0f * c6, c6x3 = 3.0f * c6;
    float xk[4][3];
    for (int a = 0; a < 3; a++) {
        xk[0][a] = x0[a];
        xk[1][a] = (x0[a] - i1[a]) + c6;
        xk[2][a] = (x0[a] - i2[a]) + c6x2;
        xk[3][a] = (x0[a] - 1.0f) + c6x3;
    }
    ix = mod289(ix);
    iy = mod289(iy);
    iz = mod289(iz);
    const float n7 = 1.0f / 7.0f;
    const float nsx = n7 * 2.0f - 0.0f, nsy = n7 * 0.5f - 1.0f, nsz = n7 * 1.0f - 0.0f;
    float out = 0.0f;
    for (int k = 0; k < 4; k++) {
        // corner k of vec4(0, i1, i2, 1)
        const float cz = k == 0 ? 0.0f : (k == 1 ? i1[2] : (k == 2 ? i2[2] : 1.0f));
        const float cy = k == 0 ? 0.0f : (k == 1 ? i1[1] : (k == 2 ? i2[1] : 1.0f));
        const float cx = k == 0 ? 0.0f : (k == 1 ? i1[0] : (k == 2 ? i2[0] : 1.0f));
        float p = permute(iz + cz);
        p = permute((p + iy) + cy);
        p = permute((p + ix) + cx);
        const float j = p - 49.0f * floorf((p * nsz) * nsz);
        const float xs = floorf(j * nsz);
        const float ys = floorf(j - 7.0f * xs);
        const float gx = xs * nsx + nsy, gy = ys * nsx + nsy;
        const float h = (1.0f - fabsf(gx)) - fabsf(gy);
        const float sh = -step(h, 0.0f);
        float ax = gx + (floorf(gx) * 2.0f + 1.0f) * sh;
        float ay = gy + (floorf(gy) * 2.0f + 1.0f) * sh;
        const float norm = 1.79284291400159f - 0.85373472095314f * ((ax * ax + ay * ay) + h * h);
        ax = ax * norm;
        ay = ay * norm;
        const float az = h * norm;
        float m = 0.6f - ((xk[k][0] * xk[k][0] + xk[k][1] * xk[k][1]) + xk[k][2] * xk[k][2]);
        m = fmaxf(m, 0.0f);
        m = m * m;
        const float d = (ax * xk[k][0] + ay * xk[k][1]) + az * xk[k][2];
        const float term = (m * m) * d;
        out = k == 0 ? term : out + term;
    }
    return 42.0f * out;
}

__device__ inline float box(float px, float py, float pz, float sx, float sy, float sz) {
    const float qx = fabsf(px) - sx, qy = fabsf(py) - sy, qz = fabsf(pz) - sz;
    const float mx = fmaxf(qx, 0.0f), my = fmaxf(qy, 0.0f), mz = fmaxf(qz, 0.0f);
    return sqrtf((mx * mx + my * my) + mz * mz) + fminf(fmaxf(fmaxf(qx, qy), qz), 0.0f);
}

__device__ inline float cone(float px, float py, float pz, float cx, float cy, float h) {
    const float qx = h * (cx / cy), qy = h * -1.0f;
    const float wx = sqrtf(px * px + pz * pz), wy = py;
    const float t = clamp01((wx * qx + wy * qy) / (qx * qx + qy * qy));
    const float ax = wx - qx * t, ay = wy - qy * t;
    const float t2 = clamp01(wx / qx);
    const float bx = wx - qx * t2, by = wy - qy * 1.0f;
    const float k = sign(qy);
    const float d = fminf(ax * ax + ay * ay, bx * bx + by * by);
    const float s = fmaxf(k * (wx * qy - wy * qx), k * (wy - qy));
    return sqrtf(d) * sign(s);
}

__device__ inline float smin(float a, float b, float k) {
    const float h = clamp01(0.5f + (0.5f * (a - b)) / k);
    return (a * (1.0f - h) + b * h) - (k * h) * (1.0f - h);
}

__device__ float eval(float px, float py, float pz) {
    float v = (0.0f + box(px, py, pz, 0.7f, 0.1f, 0.7f)) - 0.1f;
    const float s = 1.6f;
    const float q1x = px * s, q1y = py * s, q1z = pz * s;
    const float base = simplex(q1x, q1y, q1z) + 0.5f * simplex(q1x * 2.0f, q1y * 2.0f, q1z * 2.0f);
    v = v + 0.07f * base;
    const float dist = sqrtf(px * px + pz * pz);
    const float cn = cone(px * 1.5f - 0.0f, py * -1.5f - 1.0f, pz * 1.5f - 0.0f, 0.5f, 0.5f, 0.9f) - 0.1f;
    v = smin(v, cn, 0.2f);
    const float q3x = px * 2.3f, q3y = py * 0.4f, q3z = pz * 2.3f;
    float spike = simplex(q3x, q3y, q3z) + 0.5f * simplex(q3x * 2.0f, q3y * 2.0f, q3z * 2.0f);
    const float hb = smoothstep(0.0f, -1.5f, py) + smoothstep(0.0f, 0.2f, py);
    spike = ((spike + 1.6f * dist) + hb * 2.0f) - 1.0f;
    return v + 0.3f * spike;
}

}  // namespace sdf

struct ChunkGeom {
    float px, py, pz;  // lower corner
    float cell;        // 2 / 2^(base_depth + chunk_depth): a cell's edge in world units (exact)
    uint32_t depth;    // chunk_depth
};

// class byte of one cell: 0 empty, 3 grass (nothing solid one voxel above), 1 stone (procedual.wgsl:189-201)
__device__ inline uint32_t classify_cell(const ChunkGeom &g, uint32_t x, uint32_t y, uint32_t z) {
    // world = pos + (cell / 2^full) * 2; the product cell * (2 / 2^full) is the same exact value
    const float wx = g.px + float(x) * g.cell, wy = g.py + float(y) * g.cell, wz = g.pz + float(z) * g.cell;
    if (!(sdf::eval(wx, wy, wz) < 0.0f)) return 0;
    return sdf::eval(wx + 0.0f, wy + g.cell, wz + 0.0f) > 0.0f ? 3u : 1u;
}

// Lane m = Morton index of the cell.  n_cells is a multiple of 64 (chunk_depth >= 2), so every wave is whole.
__global__ __launch_bounds__(kThreads) void proc_classify_kernel(ChunkGeom g, uint32_t n_cells, uint8_t *cls, uint8_t *parent_masks) {
    const uint32_t m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= n_cells) return;
    uint32_t x, y, z;
    morton_decode(m, g.depth, x, y, z);
    const uint32_t c = classify_cell(g, x, y, z);
    cls[m] = (uint8_t)c;
    // bit i of the ballot = lane i = child (i & 7) of parent (m >> 3): byte j is parent j's child mask
    const uint64_t solid = __ballot(c != 0u);
    if ((threadIdx.x & 63u) == 0) reinterpret_cast<uint64_t *>(parent_masks)[m >> 6] = solid;
}

__device__ inline uint32_t nonzero_bytes(uint32_t w) {  // bit 8k set iff byte k of w is non-zero
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return w & 0x01010101u;
}

// mask of parent p at level L-1 from the 8 child masks of level L
__global__ __launch_bounds__(kThreads) void proc_reduce_kernel(const uint8_t *child_masks, uint32_t n_parents, uint8_t *parent_masks) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_parents) return;
    const uint2 v = reinterpret_cast<const uint2 *>(child_masks)[p];
    const uint32_t lo = nonzero_bytes(v.x), hi = nonzero_bytes(v.y);
    uint32_t mask = 0;
    for (int c = 0; c < 4; c++) mask |= ((lo >> (8 * c)) & 1u) << c | ((hi >> (8 * c)) & 1u) << (c + 4);
    parent_masks[p] = (uint8_t)mask;
}

// The ranks as a tile pass (svo_scan.h) over a level's mask bytes, which are zero-padded to whole tiles: a thread's
// kPer masks are one uint4, and the interior nodes (non-zero masks) are counted.
static_assert(kTile == kThreads * sizeof(uint4), "a tile is kThreads uint4 loads of mask bytes");
struct LevelMasks {
    const uint8_t *masks;
    __device__ uint4 load(uint32_t i0, uint32_t) const { return reinterpret_cast<const uint4 *>(masks)[i0 / kPer]; }
    __device__ uint32_t count(const uint4 &q) const {
        return __popc(nonzero_bytes(q.x)) + __popc(nonzero_bytes(q.y)) + __popc(nonzero_bytes(q.z)) + __popc(nonzero_bytes(q.w));
    }
};

// every node's exclusive rank among the interior nodes of its level
struct WriteRanks {
    uint32_t *rank;
    __device__ void operator()(const LevelMasks &, uint32_t i0, const uint4 &q, uint32_t r) const {
        const uint32_t w[4] = {nonzero_bytes(q.x), nonzero_bytes(q.y), nonzero_bytes(q.z), nonzero_bytes(q.w)};
        uint4 *out = reinterpret_cast<uint4 *>(rank + i0);
        for (int k = 0; k < 4; k++) {
            uint4 o;
            o.x = r; r += w[k] & 1u;
            o.y = r; r += (w[k] >> 8) & 1u;
            o.z = r; r += (w[k] >> 16) & 1u;
            o.w = r; r += (w[k] >> 24) & 1u;
            out[k] = o;
        }
    }
};

// One lane per node p of level L-1: an interior p owns the group base_l + 8 * rank(p) of level L.  Its 8 words: an
// interior child's pointer (base_next + 8 * its rank), CHUNK_OFFSET + class at the last level, CHUNK_OFFSET when empty.
// Nodes are written in the 8-byte <id>.bin layout (pointer, r g b = 0, pad = 0).
__global__ __launch_bounds__(kThreads) void proc_emit_kernel(const uint8_t *parent_masks, const uint32_t *parent_rank, uint32_t n_parents,
                                                       const uint8_t *child_bytes, const uint32_t *child_rank, uint32_t last,
                                                       uint32_t base_l, uint32_t base_next, uint32_t n_nodes, uint4 *out) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_parents || parent_masks[p] == 0) return;
    const uint32_t dst = base_l + 8u * parent_rank[p];
    if (dst + 8u > n_nodes) return;  // (cannot happen: the ranks and n_nodes come from the same counts)
    const uint2 cb = reinterpret_cast<const uint2 *>(child_bytes)[p];
    uint32_t w[8];
    for (int c = 0; c < 8; c++) {
        const uint32_t b = ((c < 4 ? cb.x : cb.y) >> (8 * (c & 3))) & 0xFFu;
        w[c] = last ? kChunkOffset + b : (b ? base_next + 8u * child_rank[8u * p + c] : kChunkOffset);
    }
    uint4 *o = out + dst / 2u;
    for (int k = 0; k < 4; k++) o[k] = make_uint4(w[2 * k], 0u, w[2 * k + 1], 0u);
}

__global__ __launch_bounds__(kThreads) void proc_sdf_kernel(const float *xyz, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    out[i] = sdf::eval(xyz[3u * i], xyz[3u * i + 1u], xyz[3u * i + 2u]);
}

// generate_world's block leaves: a leaf SVO_CHUNK_OFFSET + b takes block b's top_mip (world.rs:249-253); table[0] = 0
struct BlockMips {
    uint32_t rgb[9];
};
__global__ __launch_bounds__(kThreads) void proc_block_mips_kernel(uint2 *nodes, uint32_t first, uint32_t count, BlockMips table) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t b = nodes[first + i].x - kChunkOffset;
    if (b < 9u) nodes[first + i].y = table.rgb[b];
}

uint64_t pad_tile(uint64_t n) { return (n + kTile - 1) / kTile * kTile; }

}  // namespace

// Per-context workspace of the generator (svo_ctx::proc).  The level buffers only grow (svo_grow): they have the room of
// the deepest chunk generated so far, and a shallower chunk lays its levels out in the same memory.
struct svo_proc_state {
    uint32_t depth = 0;       // chunk_depth the level buffers are laid out for
    svo_dev<uint8_t> cls;     // 8^depth class bytes, Morton order
    svo_dev<uint8_t> masks;   // levels 0 .. depth-1: child masks, each level zero-padded to whole tiles
    svo_dev<uint32_t> ranks;  // levels 0 .. depth-1: exclusive ranks of the interior nodes
    svo_dev<uint32_t> tiles;  // levels 0 .. depth-1: tile counts, then tile offsets
    svo_mirrored<> totals;      // interior nodes per level
    size_t mask_bytes = 0;  // of `masks`, in use by the layout of `depth`
    uint64_t mask_off[10] = {}, rank_off[10] = {}, tile_off[10] = {};
    uint32_t n_tiles[10] = {};
    svo_dev<uint4> out;  // emitted nodes, 8 bytes each
    svo_pinned<uint8_t> stage;  // read-back buffer
    svo_events<4> ev;
    svo_events<2> mev;  // svo_world_generate: around a chunk's device mips
    float ms[SVO_PROC_TIMES] = {};

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, ev.create());
        HIP_TRY(ctx, mev.create());
        return totals.alloc(ctx, 16);
    }
};

namespace {

int check_params(svo_ctx *ctx, const svo_proc_params *p) {
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (p->chunk_depth < 2 || p->chunk_depth > 9)
        return svo_fail(ctx, SVO_ERR_ARG, "chunk_depth must be 2..9 (got " + std::to_string(p->chunk_depth) + ")");
    if (p->base_depth > 21) return svo_fail(ctx, SVO_ERR_ARG, "base_depth must be <= 21");
    return SVO_OK;
}

ChunkGeom geom_of(const svo_proc_params *p) {
    ChunkGeom g;
    g.px = p->pos[0];
    g.py = p->pos[1];
    g.pz = p->pos[2];
    g.cell = 2.0f / float(1u << (p->base_depth + p->chunk_depth));
    g.depth = p->chunk_depth;
    return g;
}

// workspace for chunks of `depth` levels (kept between calls; grown for a deeper chunk)
int ensure_state(svo_ctx *ctx, uint32_t depth) {
    if (int rc = svo_workspace_ensure(ctx, ctx->proc)) return rc;
    svo_proc_state *s = ctx->proc.get();
    if (s->depth == depth) return SVO_OK;
    s->depth = 0;  // (until the buffers have room for the new layout)
    uint64_t mb = 0, rb = 0, tb = 0;
    for (uint32_t l = 0; l < depth; l++) {
        const uint64_t n = pad_tile(1ull << (3 * l));
        s->mask_off[l] = mb;
        s->rank_off[l] = rb;
        s->tile_off[l] = tb;
        s->n_tiles[l] = (uint32_t)(n / kTile);
        mb += n;
        rb += n;
        tb += n / kTile;
    }
    s->mask_bytes = mb;
    int rc = svo_grow(ctx, (size_t)1 << (3 * depth), &s->cls);
    if (!rc) rc = svo_grow(ctx, mb, &s->masks);
    if (!rc) rc = svo_grow(ctx, rb, &s->ranks);
    if (!rc) rc = svo_grow(ctx, tb, &s->tiles);
    if (rc) return rc;
    s->depth = depth;
    return SVO_OK;
}

int launch_classify(svo_ctx *ctx, const svo_proc_params *p) {
    svo_proc_state *s = ctx->proc.get();
    const uint32_t n_cells = 1u << (3 * p->chunk_depth);
    HIP_TRY(ctx, hipMemsetAsync(s->masks, 0, s->mask_bytes, ctx->stream));
    proc_classify_kernel<<<svo_div_up(n_cells, kThreads), kThreads, 0, ctx->stream>>>(geom_of(p), n_cells, s->cls,
                                                                         s->masks + s->mask_off[p->chunk_depth - 1]);
    HIP_TRY(ctx, hipGetLastError());
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_proc_sdf(svo_ctx *ctx, const float *xyz, size_t n, float *out) {
    if (!ctx) return SVO_ERR_ARG;
    if ((!xyz || !out) && n) return svo_fail(ctx, SVO_ERR_ARG, "null points or output");
    if (n > (1ull << 28)) return svo_fail(ctx, SVO_ERR_ARG, "at most 2^28 points per call");
    if (!n) return SVO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    svo_dev<float> d;  // the points, then the distances
    HIP_TRY(ctx, d.alloc(n * 4));
    hipError_t e = hipMemcpyAsync(d, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        proc_sdf_kernel<<<svo_div_up(n, kThreads), kThreads, 0, ctx->stream>>>(d, (uint32_t)n, d + 3 * n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + 3 * n, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? SVO_OK : svo_fail_hip(ctx, e, "svo_proc_sdf");
}

int svo_proc_classify(svo_ctx *ctx, const svo_proc_params *params, uint8_t *cells_out) {
    if (!ctx) return SVO_ERR_ARG;
    int rc = check_params(ctx, params);
    if (rc) return rc;
    if (!cells_out) return svo_fail(ctx, SVO_ERR_ARG, "null output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_state(ctx, params->chunk_depth))) return rc;
    if ((rc = launch_classify(ctx, params))) return rc;
    const uint32_t d = params->chunk_depth, side = 1u << d, n = 1u << (3 * d);
    std::vector<uint8_t> morton(n);
    HIP_TRY(ctx, hipMemcpyAsync(morton.data(), ctx->proc->cls, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the reference's id order: id = x + side * y + side^2 * z (procedual.wgsl:160-170)
    for (uint32_t z = 0; z < side; z++)
        for (uint32_t y = 0; y < side; y++)
            for (uint32_t x = 0; x < side; x++) cells_out[x + side * y + side * side * z] = morton[morton_encode(x, y, z, d)];
    return SVO_OK;
}

}  // extern "C"

namespace {

// svo_proc_generate_chunk up to the emitted nodes: s->out holds *n_nodes_out nodes (0: no solid cell) in the <id>.bin
// layout, level L at base[L] .. base[L + 1]; ms[0..3] are set but for the events' [0..2].
int emit_chunk(svo_ctx *ctx, const svo_proc_params *params, double t0, uint64_t base[11], uint64_t *n_nodes_out) {
    *n_nodes_out = 0;
    const uint64_t max_nodes = params->max_nodes ? params->max_nodes : kDefaultMaxNodes;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_state(ctx, params->chunk_depth);
    if (rc) return rc;
    svo_proc_state *s = ctx->proc.get();
    const uint32_t depth = params->chunk_depth;

    HIP_TRY(ctx, hipEventRecord(s->ev[0], ctx->stream));
    if ((rc = launch_classify(ctx, params))) return rc;
    HIP_TRY(ctx, hipEventRecord(s->ev[1], ctx->stream));
    // occupancy pyramid: level L-1's masks from level L's
    for (uint32_t l = depth - 1; l >= 1; l--) {
        const uint32_t n_par = 1u << (3 * (l - 1));
        proc_reduce_kernel<<<svo_div_up(n_par, kThreads), kThreads, 0, ctx->stream>>>(s->masks + s->mask_off[l], n_par, s->masks + s->mask_off[l - 1]);
        HIP_TRY(ctx, hipGetLastError());
    }
    // ranks of the interior nodes of every level, and their counts
    for (uint32_t l = 0; l < depth; l++) {
        const uint32_t nt = s->n_tiles[l];
        if ((rc = svo_tile_pass(ctx, LevelMasks{s->masks + s->mask_off[l]}, WriteRanks{s->ranks + s->rank_off[l]}, nt, nullptr, nt * kTile,
                                s->tiles + s->tile_off[l], s->totals.dev + l)))
            return rc;
    }
    HIP_TRY(ctx, hipEventRecord(s->ev[2], ctx->stream));
    if ((rc = s->totals.read(ctx, depth))) return rc;

    // breadth-first bases: level 1 (the root group) at 0, level L+1 behind level L's 8 * interior(L-1) nodes
    base[0] = base[1] = 0;
    for (uint32_t l = 1; l <= depth; l++) base[l + 1] = base[l] + 8ull * s->totals.host()[l - 1];
    const uint64_t n_nodes = base[depth + 1];
    if (s->totals.host()[0] == 0) {  // no solid cell: the reference's "len <= 8 -> None" (procedural.rs:167)
        s->ms[0] = s->ms[1] = s->ms[2] = s->ms[4] = s->ms[5] = 0.0f;
        s->ms[3] = float(svo_now_ms() - t0);
        return SVO_OK;
    }
    if (n_nodes > max_nodes)
        return svo_fail(ctx, SVO_ERR_CAP, "chunk needs " + std::to_string(n_nodes) + " nodes, over max_nodes = " +
                                              std::to_string(max_nodes) + " (the reference panics here, procedural.rs:171-172)");
    const size_t bytes = n_nodes * 8;
    if ((rc = svo_grow(ctx, bytes / sizeof(uint4), &s->out))) return rc;
    for (uint32_t l = 1; l <= depth; l++) {
        const uint32_t n_par = 1u << (3 * (l - 1));
        const bool last = l == depth;
        proc_emit_kernel<<<svo_div_up(n_par, kThreads), kThreads, 0, ctx->stream>>>(
            s->masks + s->mask_off[l - 1], s->ranks + s->rank_off[l - 1], n_par, last ? s->cls : s->masks + s->mask_off[l],
            last ? nullptr : s->ranks + s->rank_off[l], last ? 1u : 0u, (uint32_t)base[l], (uint32_t)base[l + 1], (uint32_t)n_nodes, s->out);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(s->ev[3], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s->ms[3] = float(svo_now_ms() - t0);
    *n_nodes_out = n_nodes;
    return SVO_OK;
}

// The emitted chunk (and whatever the stream did to it since) into the pinned stage, grown to hold it; blocking.
int read_stage(svo_ctx *ctx, size_t bytes) {
    svo_proc_state *s = ctx->proc.get();
    int rc = svo_grow_pinned(ctx, bytes, &s->stage);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s->stage, s->out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_proc_generate_chunk(svo_ctx *ctx, const svo_proc_params *params, svo_cpu_octree **out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!out) return svo_fail(ctx, SVO_ERR_ARG, "null output");
    *out = nullptr;
    int rc = check_params(ctx, params);
    if (rc) return rc;
    const double t0 = svo_now_ms();
    uint64_t base[11], n_nodes = 0;
    if ((rc = emit_chunk(ctx, params, t0, base, &n_nodes))) return rc;
    if (!n_nodes) return SVO_OK;
    svo_proc_state *s = ctx->proc.get();
    const size_t bytes = n_nodes * 8;
    const double t1 = svo_now_ms();
    if ((rc = read_stage(ctx, bytes))) return rc;
    const double t2 = svo_now_ms();
    char why[128] = "";
    *out = svo_cpu_octree_from_bin(s->stage, bytes, why, sizeof why);
    if (!*out) return svo_fail(ctx, SVO_ERR_STATE, std::string("emitted tree rejected: ") + why);
    const double t3 = svo_now_ms();
    HIP_TRY(ctx, hipEventElapsedTime(&s->ms[0], s->ev[0], s->ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&s->ms[1], s->ev[1], s->ev[2]));
    HIP_TRY(ctx, hipEventElapsedTime(&s->ms[2], s->ev[2], s->ev[3]));
    s->ms[4] = float(t2 - t1);
    s->ms[5] = float(t3 - t2);
    return SVO_OK;
}

int svo_proc_timing(svo_ctx *ctx, float ms_out[SVO_PROC_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->proc) return svo_fail(ctx, SVO_ERR_STATE, "no chunk generated on this context yet");
    memcpy(ms_out, ctx->proc->ms, sizeof ctx->proc->ms);
    return SVO_OK;
}

// World::generate_world (world.rs:63-139) without its "delete the directory if it is called tmp" rule.
int svo_world_generate(svo_ctx *ctx, svo_world *w, uint32_t world_depth, uint32_t chunk_depth) {
    if (!ctx) return SVO_ERR_ARG;
    if (!w) return svo_fail(ctx, SVO_ERR_ARG, "null world");
    if (world_depth < 1 || world_depth > 4) return svo_fail(ctx, SVO_ERR_ARG, "world_depth must be 1..4");
    if (chunk_depth < 2 || chunk_depth > 9) return svo_fail(ctx, SVO_ERR_ARG, "chunk_depth must be 2..9");
    for (uint32_t b = 1; b <= 8; b++)  // mips of block leaves need the blocks' top_mip (World::new, world.rs:19-58)
        if (!svo_world_chunk(w, b)) return svo_fail(ctx, SVO_ERR_STATE, "block " + std::to_string(b) + " is not loaded (insert blocks 1..8 first)");
    svo_world_writer world(ctx, w, world_depth);  // (the directory is made before any GPU work)
    int rc = world.create();
    if (rc) return rc;
    float times[4] = {0, 0, 0, 0};  // GPU, read-back, mips, writes
    BlockMips blocks{};  // block leaves take their block's top_mip (as svo_world_generate_mip_tree does)
    for (uint32_t b = 1; b <= 8; b++) {
        uint8_t rgb[3];
        svo_cpu_octree_top_mip(svo_world_chunk(w, b), rgb);
        blocks.rgb[b] = rgb[0] | rgb[1] << 8 | rgb[2] << 16;
    }
    const uint32_t n = 1u << world_depth;
    const float voxel = 2.0f / float(n);
    uint32_t i = 0;
    for (uint32_t x = 0; x < n; x++)
        for (uint32_t y = 0; y < n; y++)
            for (uint32_t z = 0; z < n; z++, i++) {
                svo_proc_params p{};
                p.pos[0] = float(x) * voxel - 1.0f;
                p.pos[1] = float(y) * voxel - 1.0f;
                p.pos[2] = float(z) * voxel - 1.0f;
                p.base_depth = world_depth;
                p.chunk_depth = chunk_depth;
                uint64_t base[11], n_nodes = 0;
                if ((rc = check_params(ctx, &p))) return rc;
                if ((rc = emit_chunk(ctx, &p, svo_now_ms(), base, &n_nodes))) return rc;
                svo_proc_state *s = ctx->proc.get();
                times[0] += s->ms[3];
                if (!n_nodes) continue;
                // mips on the device: block leaves first, then the interior levels bottom-up
                uint2 *nodes = reinterpret_cast<uint2 *>(s->out.get());
                HIP_TRY(ctx, hipEventRecord(s->mev[0], ctx->stream));
                const uint32_t leaves = uint32_t(base[chunk_depth + 1] - base[chunk_depth]);
                proc_block_mips_kernel<<<svo_div_up(leaves, kThreads), kThreads, 0, ctx->stream>>>(nodes, (uint32_t)base[chunk_depth], leaves, blocks);
                for (uint32_t l = chunk_depth - 1; l >= 1; l--) {
                    const uint32_t count = uint32_t(base[l + 1] - base[l]);
                    mip_level_kernel<<<svo_div_up(count, kThreads), kThreads, 0, ctx->stream>>>(nodes, (uint32_t)base[l], count, (uint32_t)n_nodes);
                }
                HIP_TRY(ctx, hipGetLastError());
                HIP_TRY(ctx, hipEventRecord(s->mev[1], ctx->stream));
                // one copy into the pinned stage; the writer takes <id>.bin and top_mip from there
                double t = svo_now_ms();
                if ((rc = read_stage(ctx, n_nodes * 8))) return rc;
                times[1] += float(svo_now_ms() - t);
                float mip_ms = 0.0f;
                HIP_TRY(ctx, hipEventElapsedTime(&mip_ms, s->mev[0], s->mev[1]));
                times[2] += mip_ms;
                t = svo_now_ms();
                if ((rc = world.add_chunk(i, s->stage, n_nodes))) return rc;
                times[3] += float(svo_now_ms() - t);
            }
    float mip_ms = 0.0f, save_ms = 0.0f;
    if ((rc = world.finish(&mip_ms, &save_ms))) return rc;
    times[2] += mip_ms;
    times[3] += save_ms;
    memcpy(ctx->proc->ms + 6, times, sizeof times);
    return SVO_OK;
}

}  // extern "C"

// svo_solid.hip -- closed triangle meshes voxelised solid on the device: the cells of the `depth` grid whose
// perturbed centre lies inside the mesh by the even-odd or the non-zero rule, as y-spans or as a voxel list.  Exact
// integers, breadth-first refinement, one stable sort, no atomics: the same bytes on every run, whatever the triangles'
// order.  One lane per item everywhere; no lane loops over a triangle's columns or over a span's cells.
//
//   setup    one lane per triangle: svo_mesh.h's check and gather, the root pair (the whole grid's square)
//   levels   (triangle, xz-square) pairs refined one level at a time, as svo_voxelize.hip refines its cells: a mask of the 4
//            child squares whose closed square meets the closed projected triangle (the bounding-box shortcut, then 2 box
//            axes and 3 edge normals in int64), the tile pass's count, the total in 64 bits, the row-wise scatter.  An
//            edge-on triangle (n.y == 0) gets the mask 0 at level 1.  The last level's mask is the exact covering test with
//            the tie rule, and its scatter emits one crossing per covering pair: key ((x << depth | z) << 22) | k, value w,
//            with the height k found by bisection on the sign of the 128-bit plane value: no division
//   sort     the crossings by key, with the builder's stable radix sort (svo_build_sort_u64)
//   spans    heads: a tile pass flags the first crossing of every column and writes the columns' first crossings and
//            every crossing's column; the in-place scan of w (non-zero rule); the open columns, counted by a tile count over
//            the columns; intervals: crossing j of the column [s, e) closes [k_(j-1), k_j) (k_(s-1) = 0), inside iff e - j is
//            odd or the sum of w over [j, e) is non-zero; a tile pass keeps the non-empty ones; runs: a tile pass over those
//            flags an inside interval that is the first of its column or follows an outside one (a start) and one that is the
//            last of its column or precedes an outside one (an end): the r-th start and the r-th end make the r-th span
//   cells    the spans' lengths summed in 64 bits, scanned in place; one lane per output cell: a tile of kTile cells finds
//            its first and last span by binary search in the offsets, keeps the offsets between them in LDS (at most kTile,
//            since a span has a cell at least), and every lane finds its span there
//
// Widths: doubled coordinates are odd and below 2^28, so edges are below 2^28, n's components and the edge functions F
// below 2^57 (int64), the plane value below 2^87 (__int128).  A key is 2 * depth + 22 bits: 64 at depth 21.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_mesh.h"
#include "svo_scan.h"

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;
constexpr uint64_t kDefaultMaxPairs = 1ull << 27;
constexpr uint32_t kHeightBits = 22;  // k lies in [0, 2^depth]: depth + 1 bits
static_assert(2 * 21 + kHeightBits == 64, "a crossing's key, (x << depth | z) << 22 | k, fills 64 bits at depth 21 exactly");
constexpr uint32_t kHeightMask = (1u << kHeightBits) - 1u;
constexpr uint32_t kInsideBit = 1u << 31;
// the words read back: the first bad triangle's verdict (svo_mesh.h), a 64-bit count in two halves (a level's pairs, the
// cells), the columns, the open columns, the non-empty intervals, the spans
enum Status { kStBad, kStCountLo, kStCountHi, kStCols, kStOpen, kStIntervals, kStSpans, kStWords };

typedef __int128 i128;

__device__ inline uint64_t square_pack(uint32_t x, uint32_t z) { return uint64_t(x) << 32 | z; }
__device__ inline uint32_t square_x(uint64_t s) { return uint32_t(s >> 32); }
__device__ inline uint32_t square_z(uint64_t s) { return uint32_t(s); }

__global__ __launch_bounds__(kThreads) void solid_setup_kernel(const uint32_t *__restrict__ vq, uint32_t n_vertices,
                                                               const uint32_t *__restrict__ tri, uint32_t n_tris, uint32_t depth,
                                                               int32_t *__restrict__ tv, uint32_t *__restrict__ pair_tri,
                                                               uint64_t *__restrict__ pair_sq, uint32_t *__restrict__ block_bad) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    uint32_t bad = kNoBadTriangle;
    if (t < n_tris) {
        int32_t v[9];
        bad = mesh_gather_triangle(vq, n_vertices, tri, t, depth, v);
        for (uint32_t k = 0; k < 9; k++) tv[9ull * t + k] = v[k];
        pair_tri[t] = t;
        pair_sq[t] = 0;
    }
    bad = block_min<kThreads>(bad);
    if (threadIdx.x == 0) block_bad[blockIdx.x] = bad;
}

__device__ inline int64_t abs64(int64_t v) { return v < 0 ? -v : v; }
__device__ inline int64_t shl(int64_t v, uint32_t k) { return int64_t(uint64_t(v) << k); }
__device__ inline int sign64(int64_t v) { return (v > 0) - (v < 0); }

// the projection of triangle v (nine doubled coordinates) onto the xz plane: edge i runs from vertex i to vertex i + 1
struct Projected {
    int32_t x[3], z[3], ex[3], ez[3];
    int64_t ny;  // n.y = e0.z e1.x - e0.x e1.z: twice the projection's signed area, against the xz orientation
    __device__ explicit Projected(const int32_t *v) {
#pragma unroll
        for (int j = 0; j < 3; j++) x[j] = v[3 * j], z[j] = v[3 * j + 2];
#pragma unroll
        for (int j = 0; j < 3; j++) ex[j] = x[(j + 1) % 3] - x[j], ez[j] = z[(j + 1) % 3] - z[j];
        ny = int64_t(ez[0]) * ex[1] - int64_t(ex[0]) * ez[1];
    }
};

// The child squares of the level-(l - 1) square (px, pz) that the projected triangle meets, closed against closed, as a
// mask by child index x * 2 + z.  hs = depth - l + 6: a child's half side is 2^hs.  The pair itself overlaps, or is a root.
__device__ inline uint32_t overlap_mask(const Projected &p, uint32_t px, uint32_t pz, uint32_t hs) {
    if (p.ny == 0) return 0u;  // edge-on
    const int32_t lo_x = min(p.x[0], min(p.x[1], p.x[2])), hi_x = max(p.x[0], max(p.x[1], p.x[2]));
    const int32_t lo_z = min(p.z[0], min(p.z[1], p.z[2])), hi_z = max(p.z[0], max(p.z[1], p.z[2]));
    const uint32_t cell_x = uint32_t(lo_x) >> (hs + 1), cell_z = uint32_t(lo_z) >> (hs + 1);
    // the cheap path: the bounding box lies in one square of level l, which then is a child of this pair's
    if (cell_x == uint32_t(hi_x) >> (hs + 1) && cell_z == uint32_t(hi_z) >> (hs + 1)) return 1u << ((cell_x & 1u) << 1 | (cell_z & 1u));

    // relative to the parent's centre: a child's centre is at (sx, sz) * h with s = +-1
    const int32_t side = 1 << (hs + 1);
    const int32_t centre_x = int32_t((2u * px + 1u) << (hs + 1)), centre_z = int32_t((2u * pz + 1u) << (hs + 1));
    const bool half_x[2] = {!(lo_x - centre_x > 0 || hi_x - centre_x < -side), !(lo_x - centre_x > side || hi_x - centre_x < 0)};
    const bool half_z[2] = {!(lo_z - centre_z > 0 || hi_z - centre_z < -side), !(lo_z - centre_z > side || hi_z - centre_z < 0)};
    // the edge normals: e.x z - e.z x has one value on the edge's two vertices and one on the third
    int64_t proj_lo[3], proj_hi[3], reach[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int k = (i + 2) % 3;
        const int64_t on = int64_t(p.ex[i]) * (p.z[i] - centre_z) - int64_t(p.ez[i]) * (p.x[i] - centre_x);
        const int64_t off = int64_t(p.ex[i]) * (p.z[k] - centre_z) - int64_t(p.ez[i]) * (p.x[k] - centre_x);
        proj_lo[i] = min(on, off);
        proj_hi[i] = max(on, off);
        reach[i] = shl(abs64(p.ex[i]) + abs64(p.ez[i]), hs);
    }
    uint32_t mask = 0;
#pragma unroll
    for (int child = 0; child < 4; child++) {
        const int sx = child & 2 ? 1 : -1, sz = child & 1 ? 1 : -1;
        bool ok = half_x[child >> 1] && half_z[child & 1];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int64_t shift = shl(int64_t(p.ex[i]) * sz - int64_t(p.ez[i]) * sx, hs);
            ok = ok && !(proj_lo[i] - shift > reach[i] || proj_hi[i] - shift < -reach[i]);
        }
        mask |= ok ? 1u << child : 0u;
    }
    return mask;
}

// The last level: the child columns of (px, pz) that the triangle covers, by the contract's rule: all three edge functions
// at the column's centre on the inner side, a zero decided as the centre moved by (dx, dz), dx >> dz > 0, decides it.
__device__ inline uint32_t cover_mask(const Projected &p, uint32_t px, uint32_t pz) {
    if (p.ny == 0) return 0u;
    const int s = p.ny < 0 ? 1 : -1;
    uint32_t mask = 0;
#pragma unroll
    for (int child = 0; child < 4; child++) {
        const int32_t cx = int32_t((2u * px + (child >> 1)) * 128u + 64u), cz = int32_t((2u * pz + (child & 1)) * 128u + 64u);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int64_t f = int64_t(p.ex[i]) * (cz - p.z[i]) - int64_t(p.ez[i]) * (cx - p.x[i]);
            const int sgn = f ? sign64(f) : p.ez[i] ? -sign64(p.ez[i]) : sign64(p.ex[i]);
            ok = ok && s * sgn > 0;
        }
        mask |= ok ? 1u << child : 0u;
    }
    return mask;
}

template <bool kLast>
__global__ __launch_bounds__(kThreads) void solid_test_kernel(const int32_t *__restrict__ tv, const uint32_t *__restrict__ pair_tri,
                                                              const uint64_t *__restrict__ pair_sq, uint32_t m, uint32_t hs,
                                                              uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const int32_t *src = tv + 9ull * pair_tri[i];
    int32_t v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = src[k];
    const Projected p(v);
    const uint64_t sq = pair_sq[i];
    mask[i] = uint8_t(kLast ? cover_mask(p, square_x(sq), square_z(sq)) : overlap_mask(p, square_x(sq), square_z(sq), hs));
}

// The tile pass's items: a level's pairs with their child masks, one byte per pair (svo_scan.h: FlagBytes).
struct Squares : FlagBytes {
    const uint32_t *tri;
    const uint64_t *sq;
};

// A total in 64 bits, before it is compared with a cap: a level's tile sums before tile_offsets_kernel scans them in
// place (4 children of up to 2^31 pairs), and the blocks' sums of the spans' lengths.
static_assert(kStCountHi == kStCountLo + 1, "block_total64 writes the two halves side by side");
template <typename T>
__global__ __launch_bounds__(kTopThreads) void solid_total_kernel(const T *sums, uint32_t n, uint32_t *status) {
    block_total64(sums, n, status + kStCountLo);
}

// The triangle's height in the column with centre (cx, cz): the number of cy in [0, 2^depth) with sign(n.y) * D(cy) < 0,
// D(cy) = n . (C - V0).  sign(n.y) * D(cy) = b + m * cy with m = 128 |n.y| > 0, so these cy are a prefix, and its length
// is found in at most depth + 1 bisection steps on the sign alone.
__device__ inline uint32_t column_height(const int32_t *v, int64_t nx, int64_t ny, int64_t nz, int32_t cx, int32_t cz, uint32_t depth) {
    const i128 a = i128(nx) * (cx - v[0]) + i128(nz) * (cz - v[2]) + i128(ny) * (64 - v[1]);
    const i128 b = ny > 0 ? a : -a;
    const i128 m = i128(abs64(ny)) * 128;
    uint32_t lo = 0, hi = 1u << depth;  // every cy < lo is below the crossing, no cy >= hi is
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (b + m * mid < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct SolidOut {
    uint32_t *pair_tri;  // the next level's pairs, or
    uint64_t *pair_sq;
    uint64_t *keys;      // (kEmit) the crossings
    uint32_t *vals;
    const int32_t *tv;
    uint32_t depth;
    uint32_t room;  // entries the outputs hold: the level's total, which the host has checked
};

// the children `bits` of pair i, in child order from output o on
template <bool kEmit>
struct Children {
    SolidOut out;
    __device__ void operator()(const Squares &p, uint32_t i, uint32_t bits, uint32_t o) const {
        const uint32_t t = p.tri[i];
        const uint64_t sq = p.sq[i];
        const uint32_t x = square_x(sq) << 1, z = square_z(sq) << 1;
        const auto each_child = [&](auto &&write) {
            for (; bits; bits &= bits - 1u, o++) {
                const uint32_t child = __ffs(bits) - 1u;
                if (o >= out.room) break;  // (never: room is the scan's total)
                write(o, x | (child >> 1), z | (child & 1u));
            }
        };
        if constexpr (kEmit) {  // (the pair scatter never loads the triangle)
            int32_t v[9];
#pragma unroll
            for (int k = 0; k < 9; k++) v[k] = out.tv[9ull * t + k];
            const int32_t e0[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e1[3] = {v[6] - v[3], v[7] - v[4], v[8] - v[5]};
            const int64_t n[3] = {int64_t(e0[1]) * e1[2] - int64_t(e0[2]) * e1[1], int64_t(e0[2]) * e1[0] - int64_t(e0[0]) * e1[2],
                                  int64_t(e0[0]) * e1[1] - int64_t(e0[1]) * e1[0]};
            each_child([&](uint32_t at, uint32_t cx, uint32_t cz) {
                const uint32_t k = column_height(v, n[0], n[1], n[2], int32_t(cx * 128u + 64u), int32_t(cz * 128u + 64u), out.depth);
                out.keys[at] = ((uint64_t(cx) << out.depth | cz) << kHeightBits) | k;
                out.vals[at] = n[1] > 0 ? 1u : 0xFFFFFFFFu;  // w = sign(n.y), two's complement
            });
        } else {
            each_child([&](uint32_t at, uint32_t cx, uint32_t cz) {
                out.pair_tri[at] = t;
                out.pair_sq[at] = square_pack(cx, cz);
            });
        }
    }
};

// ---- spans ----
// The sorted crossings: keys[0, n), and for the non-zero rule wsum[0, n], the exclusive scan of their w (wrapping u32:
// differences are exact).  head[c] is column c's first crossing, col[j] crossing j's column, *n_cols their number.
struct Crossings {
    const uint64_t *keys;
    const uint32_t *wsum;
    uint32_t *head, *col;
    const uint32_t *n_cols;
    uint32_t n, nonzero;
    __device__ uint32_t column_end(uint32_t c, uint32_t cols) const { return c + 1 < cols ? head[c + 1] : n; }
    // whether the crossings [j, e) leave a cell below them inside
    __device__ bool inside(uint32_t j, uint32_t e) const { return nonzero ? wsum[e] != wsum[j] : (e - j) & 1u; }
};

// items: the crossings; flagged: the first of a column
struct Heads {
    Crossings c;
    __device__ uint32_t load(uint32_t i0, uint32_t m) const {
        if (i0 >= m) return 0u;
        uint32_t mask = 0;
        uint64_t prev = i0 ? c.keys[i0 - 1] >> kHeightBits : ~0ull;
        for (uint32_t k = 0; k < kPer && i0 + k < m; k++) {
            const uint64_t column = c.keys[i0 + k] >> kHeightBits;
            mask |= uint32_t(column != prev) << k;
            prev = column;
        }
        return mask;
    }
    __device__ uint32_t count(uint32_t mask) const { return __popc(mask); }
    __device__ void operator()(const Heads &, uint32_t i0, uint32_t mask, uint32_t rank) const {
        for (uint32_t k = 0; k < kPer && i0 + k < c.n; k++) {
            if (mask >> k & 1u) {
                if (rank < c.n) c.head[rank] = i0 + k;
                rank++;
            }
            c.col[i0 + k] = rank - 1u;  // (crossing 0 is a head: rank >= 1)
        }
    }
};

// items: the columns; flagged: the open ones
struct OpenColumns {
    Crossings c;
    __device__ uint32_t load(uint32_t i0, uint32_t m) const {
        uint32_t mask = 0;
        for (uint32_t k = 0; k < kPer && i0 + k < m; k++) mask |= uint32_t(c.inside(c.head[i0 + k], c.column_end(i0 + k, m))) << k;
        return mask;
    }
    __device__ uint32_t count(uint32_t mask) const { return __popc(mask); }
};

// items: the crossings, each as the interval it closes; flagged: the non-empty ones.  Kept as key = column << 22 | y0 and
// y1 | kInsideBit.
struct Intervals {
    Crossings c;
    uint64_t *iv_key;
    uint32_t *iv_y1;
    // where the interval that `key` closes begins: the height of the crossing before it when that is the same column's
    // (crossing 0 has none: depth 21's last column is all ones, so no key value can stand for "none")
    __device__ static uint32_t begin(uint64_t key, uint64_t prev, bool has_prev) {
        return has_prev && key >> kHeightBits == prev >> kHeightBits ? uint32_t(prev) & kHeightMask : 0u;
    }
    __device__ uint32_t load(uint32_t i0, uint32_t m) const {
        if (i0 >= m) return 0u;
        uint32_t mask = 0;
        uint64_t prev = i0 ? c.keys[i0 - 1] : 0ull;
        for (uint32_t k = 0; k < kPer && i0 + k < m; k++) {
            const uint64_t key = c.keys[i0 + k];
            mask |= uint32_t(begin(key, prev, i0 + k > 0) < (uint32_t(key) & kHeightMask)) << k;
            prev = key;
        }
        return mask;
    }
    __device__ uint32_t count(uint32_t mask) const { return __popc(mask); }
    __device__ void operator()(const Intervals &, uint32_t i0, uint32_t mask, uint32_t rank) const {
        const uint32_t cols = *c.n_cols;
        for (uint32_t k = 0; k < kPer && i0 + k < c.n; k++) {
            if (!(mask >> k & 1u)) continue;
            const uint32_t j = i0 + k;
            const uint64_t key = c.keys[j];
            const uint32_t y0 = begin(key, j ? c.keys[j - 1] : 0ull, j > 0);
            if (rank < c.n) {
                iv_key[rank] = (key & ~uint64_t(kHeightMask)) | y0;
                iv_y1[rank] = (uint32_t(key) & kHeightMask) | (c.inside(j, c.column_end(c.col[j], cols)) ? kInsideBit : 0u);
            }
            rank++;
        }
    }
};

// items: the non-empty intervals (consecutive ones of a column touch); state: the starts of runs of inside intervals in the
// low half, their ends in the high half; counted: the starts.  The emit writes (x, z, y0) at a start's rank and y1 at the
// rank of the last start before an end, which is that run's.
struct Runs {
    const uint64_t *iv_key;
    const uint32_t *iv_y1;
    uint32_t *spans;  // (emit) 4 u32 per span
    uint32_t room, depth;
    __device__ uint32_t load(uint32_t i0, uint32_t m) const {
        if (i0 >= m) return 0u;
        uint32_t state = 0;
        // (column, inside) of the items i - 1, i, i + 1; none: a column that no interval has
        const auto at = [&](uint32_t i) { return i < m ? (iv_key[i] >> kHeightBits) << 1 | (iv_y1[i] >> 31) : ~0ull; };
        uint64_t prev = i0 ? at(i0 - 1) : ~0ull, cur = at(i0);
        for (uint32_t k = 0; k < kPer && i0 + k < m; k++) {
            const uint64_t next = at(i0 + k + 1);
            if (cur & 1u) {
                state |= uint32_t(prev != cur) << k;  // the same column's inside interval before it: not a start
                state |= uint32_t(next != cur) << (16 + k);
            }
            prev = cur;
            cur = next;
        }
        return state;
    }
    __device__ uint32_t count(uint32_t state) const { return __popc(state & 0xFFFFu); }
    __device__ void operator()(const Runs &, uint32_t i0, uint32_t state, uint32_t rank) const {
        for (uint32_t k = 0; k < kPer; k++) {
            if (state >> k & 1u) {
                const uint64_t key = iv_key[i0 + k];
                if (rank < room) {
                    spans[4ull * rank] = uint32_t(key >> (kHeightBits + depth));
                    spans[4ull * rank + 1] = uint32_t(key >> kHeightBits) & ((1u << depth) - 1u);
                    spans[4ull * rank + 2] = uint32_t(key) & kHeightMask;
                }
                rank++;
            }
            if ((state >> (16 + k) & 1u) && rank - 1u < room) spans[4ull * (rank - 1u) + 3] = iv_y1[i0 + k] & ~kInsideBit;
        }
    }
};

// ---- cells ----
// off[r] = span r's length, and the block's sum of them in 64 bits (a span is up to 2^21 cells, a grid up to 2^63)
__global__ __launch_bounds__(kThreads) void solid_lengths_kernel(const uint32_t *__restrict__ spans, uint32_t n_spans,
                                                                 uint32_t *__restrict__ off, uint64_t *__restrict__ block_sum) {
    __shared__ uint64_t s[kThreads];
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    uint32_t len = 0;
    if (r < n_spans) off[r] = len = spans[4ull * r + 3] - spans[4ull * r + 2];
    s[threadIdx.x] = len;
    __syncthreads();
    for (uint32_t step = kThreads / 2; step > 0; step >>= 1) {
        if (threadIdx.x < step) s[threadIdx.x] += s[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sum[blockIdx.x] = s[0];
}

// the last r in [0, n) with off[r] <= v (off[0] = 0)
__device__ inline uint32_t last_at_most(const uint32_t *off, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane per output cell, a block per kTile cells.  off: the spans' first cells (the exclusive scan of their lengths).
__global__ __launch_bounds__(kThreads) void solid_cells_kernel(const uint32_t *__restrict__ spans, const uint32_t *__restrict__ off,
                                                               uint32_t n_spans, uint32_t total, uint32_t *__restrict__ out) {
    __shared__ uint32_t s_off[kTile];
    __shared__ uint32_t s_span[2];
    const uint32_t tile0 = blockIdx.x * kTile, tile_end = min(tile0 + kTile, total);
    if (tile0 >= total) return;
    // two waves search at the same time
    if (threadIdx.x == 0) s_span[0] = last_at_most(off, n_spans, tile0);
    if (threadIdx.x == 64) s_span[1] = last_at_most(off, n_spans, tile_end - 1u);
    __syncthreads();
    const uint32_t first = s_span[0], n_here = min(s_span[1] - first + 1u, kTile);  // (every span has a cell: at most kTile)
    for (uint32_t i = threadIdx.x; i < n_here; i += kThreads) s_off[i] = off[first + i];
    __syncthreads();
    for (uint32_t o = tile0 + threadIdx.x; o < tile_end; o += kThreads) {
        const uint32_t i = last_at_most(s_off, n_here, o);
        const uint32_t *span = spans + 4ull * (first + i);
        out[3ull * o] = span[0];
        out[3ull * o + 1] = span[2] + (o - s_off[i]);
        out[3ull * o + 2] = span[1];
    }
}

enum Ev { kEvStart, kEvSetup, kEvLevels, kEvSort, kEvSpans, kEvEmit, kEvs };

}  // namespace

// Per-context workspace of the solid voxeliser (svo_ctx::solid): nine i32 per triangle; two pair arrays of twelve bytes
// per pair that take turns and one mask byte per pair; per crossing a key, a value, a column, a head, and an interval of
// twelve bytes; per span 16 bytes and an offset; one u32 per tile and one u64 per block of spans.
struct svo_solid_state {
    svo_dev<int32_t> tv;
    svo_dev<uint32_t> pair_tri[2];
    svo_dev<uint64_t> pair_sq[2];
    svo_dev<uint8_t> mask;
    svo_dev<uint32_t> tiles;
    svo_dev<uint64_t> keys, iv_key;
    svo_dev<uint32_t> vals, head, col, iv_y1;
    svo_dev<uint32_t> spans, off;
    svo_dev<uint64_t> block_sum;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_SOLID_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
};

extern "C" {

int svo_mesh_voxelize_solid(svo_ctx *ctx, const svo_solid_params *p, const uint32_t *vq_dev, const uint32_t *tri_dev, size_t n_tris,
                            uint32_t *out_dev, uint64_t *n_out, uint64_t *n_open_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    int rc = svo_check_flags(ctx, p->flags, SVO_SOLID_NONZERO | SVO_SOLID_SPANS);
    if (rc) return rc;
    if (p->reserved) return svo_fail(ctx, SVO_ERR_ARG, "reserved must be 0 (got " + std::to_string(p->reserved) + ")");
    if ((rc = svo_check_depth(ctx, p->depth, 21))) return rc;
    if (n_tris >= kMaxEntries) return svo_fail(ctx, SVO_ERR_ARG, "n_tris must be below 2^31 (got " + std::to_string(n_tris) + ")");
    if (n_tris && !vq_dev) return svo_fail(ctx, SVO_ERR_ARG, "null vq_dev");
    if (n_tris && !tri_dev) return svo_fail(ctx, SVO_ERR_ARG, "null tri_dev");
    if (!n_tris) {
        *n_out = 0;
        if (n_open_out) *n_open_out = 0;
        return SVO_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t depth = p->depth, n = (uint32_t)n_tris;
    const bool nonzero = p->flags & SVO_SOLID_NONZERO, as_spans = p->flags & SVO_SOLID_SPANS;
    if ((rc = svo_workspace_ensure(ctx, ctx->solid))) return rc;
    svo_solid_state *s = ctx->solid.get();
    if ((rc = s->timer.begin(ctx))) return rc;
    const uint32_t *st = s->status.host();
    const uint64_t max_pairs = std::min<uint64_t>(p->max_pairs ? p->max_pairs : kDefaultMaxPairs, kMaxEntries - 1);
    const uint64_t cap = out_dev ? std::min<uint64_t>(p->max_out, kMaxEntries - 1) : kMaxEntries - 1;
    const auto over_cap = [&](uint64_t count, const char *noun) {
        return svo_fail(ctx, SVO_ERR_CAP, "the mesh has " + std::to_string(count) + " " + noun + ", " +
                                              (count >= kMaxEntries ? "2^31 or more" : "more than max_out = " + std::to_string(p->max_out)));
    };

    // setup: the check, the gather, the root pairs
    const uint32_t n_blocks = svo_div_up(n, kThreads);
    if ((rc = svo_grow(ctx, 9 * (size_t)n, &s->tv))) return rc;
    if ((rc = svo_grow(ctx, (size_t)n, &s->pair_tri[0], &s->pair_sq[0]))) return rc;
    if ((rc = svo_grow(ctx, (size_t)n_blocks, &s->tiles))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    solid_setup_kernel<<<n_blocks, kThreads, 0, ctx->stream>>>(vq_dev, p->n_vertices, tri_dev, n, depth, s->tv, s->pair_tri[0],
                                                               s->pair_sq[0], s->tiles);
    min_of_blocks_kernel<1><<<1, kTopThreads, 0, ctx->stream>>>(s->tiles, n_blocks, s->status.dev + kStBad);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvSetup));

    // the column levels; the last one emits the crossings
    uint32_t m = n, cur = 0, n_cross = 0;  // the pairs of level l - 1: pair_*[cur][0, m)
    for (uint32_t l = 1; l <= depth; l++) {
        const bool last = l == depth;
        const uint32_t n_tiles = svo_div_up(m, kTile), hs = depth - l + SVO_VOX_SUBBITS;
        if ((rc = svo_grow(ctx, size_t(n_tiles) * kTile, &s->mask))) return rc;
        if ((rc = svo_grow(ctx, (size_t)n_tiles, &s->tiles))) return rc;
        const Squares pairs{{s->mask}, s->pair_tri[cur], s->pair_sq[cur]};
        if (last) solid_test_kernel<true><<<svo_div_up(m, kThreads), kThreads, 0, ctx->stream>>>(s->tv, pairs.tri, pairs.sq, m, hs, s->mask);
        else solid_test_kernel<false><<<svo_div_up(m, kThreads), kThreads, 0, ctx->stream>>>(s->tv, pairs.tri, pairs.sq, m, hs, s->mask);
        tile_count_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(pairs, nullptr, m, s->tiles);
        solid_total_kernel<<<1, kTopThreads, 0, ctx->stream>>>(s->tiles.get(), n_tiles, s->status.dev.get());
        tile_offsets_kernel<<<1, kTopThreads, 0, ctx->stream>>>(s->tiles, n_tiles, nullptr, 0, nullptr);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = s->status.read(ctx))) return rc;
        if (l == 1 && st[kStBad] != kNoBadTriangle) return svo_fail(ctx, SVO_ERR_ARG, mesh_bad_triangle(st[kStBad], depth, p->n_vertices));
        const uint64_t count = uint64_t(st[kStCountHi]) << 32 | st[kStCountLo];
        if (count > max_pairs)
            return svo_fail(ctx, SVO_ERR_CAP, "level " + std::to_string(l) + " has " + std::to_string(count) +
                                                  (last ? " crossings" : " (triangle, square) pairs") + ", more than max_pairs = " +
                                                  std::to_string(max_pairs));
        SolidOut out{};
        out.room = (uint32_t)count;
        if (!count) break;  // (every triangle edge-on, or no centre covered)
        if (!last) {
            const uint32_t next = cur ^ 1u;
            if ((rc = svo_grow(ctx, (size_t)count, &s->pair_tri[next], &s->pair_sq[next]))) return rc;
            out.pair_tri = s->pair_tri[next];
            out.pair_sq = s->pair_sq[next];
            tile_scatter_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(pairs, Children<false>{out}, m, s->tiles);
            HIP_TRY(ctx, hipGetLastError());
            m = (uint32_t)count;
            cur = next;
            continue;
        }
        n_cross = (uint32_t)count;
        if ((rc = svo_grow(ctx, (size_t)n_cross, &s->keys))) return rc;
        if ((rc = svo_grow(ctx, (size_t)n_cross + 1, &s->vals))) return rc;  // (and the scan's total)
        out.keys = s->keys;
        out.vals = s->vals;
        out.tv = s->tv;
        out.depth = depth;
        tile_scatter_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(pairs, Children<true>{out}, m, s->tiles);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvLevels));

    // the sorted crossings: in this workspace or in the builder's (both with room for the scan's total behind them)
    uint64_t *keys = s->keys;
    uint32_t *vals = s->vals;
    if (n_cross && (rc = svo_build_sort_u64(ctx, &keys, &vals, n_cross, 2 * depth + kHeightBits))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvSort));

    uint64_t count = 0;
    uint32_t n_spans = 0, n_open = 0;
    if (n_cross) {
        const uint32_t n_tiles = svo_div_up(n_cross, kTile);
        if ((rc = svo_grow(ctx, (size_t)n_tiles, &s->tiles))) return rc;
        if ((rc = svo_grow(ctx, (size_t)n_cross, &s->head, &s->col, &s->iv_y1))) return rc;
        if ((rc = svo_grow(ctx, (size_t)n_cross, &s->iv_key))) return rc;
        uint32_t *status = s->status.dev;
        const Crossings c{keys, vals, s->head, s->col, status + kStCols, n_cross, nonzero};
        if ((rc = svo_tile_pass(ctx, Heads{c}, Heads{c}, n_tiles, nullptr, n_cross, s->tiles, status + kStCols))) return rc;
        if (nonzero) {
            HIP_TRY(ctx, hipMemsetAsync(vals + n_cross, 0, sizeof(uint32_t), ctx->stream));
            if ((rc = svo_scan_u32(ctx, vals, n_cross + 1))) return rc;
        }
        if ((rc = svo_tile_count(ctx, OpenColumns{c}, n_tiles, status + kStCols, n_cross, s->tiles, status + kStOpen))) return rc;
        const Intervals intervals{c, s->iv_key, s->iv_y1};
        if ((rc = svo_tile_pass(ctx, intervals, intervals, n_tiles, nullptr, n_cross, s->tiles, status + kStIntervals))) return rc;
        Runs runs{s->iv_key, s->iv_y1, nullptr, 0, depth};
        if ((rc = svo_tile_count(ctx, runs, n_tiles, status + kStIntervals, n_cross, s->tiles, status + kStSpans))) return rc;
        if ((rc = s->status.read(ctx))) return rc;
        n_spans = st[kStSpans];
        n_open = st[kStOpen];
        count = n_spans;
        if (as_spans && count > cap) return over_cap(count, "spans");
        // the spans: into the caller's output, or for the cells into the workspace (s->tiles still holds the runs' offsets)
        runs.room = n_spans;
        if (as_spans) runs.spans = out_dev;
        else if (n_spans) {
            if ((rc = svo_grow(ctx, 4 * (size_t)n_spans, &s->spans))) return rc;
            if ((rc = svo_grow(ctx, (size_t)n_spans, &s->off))) return rc;
            if ((rc = svo_grow(ctx, (size_t)svo_div_up(n_spans, kThreads), &s->block_sum))) return rc;
            runs.spans = s->spans;
        }
        if (!as_spans && n_spans) {
            tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(runs, runs, status + kStIntervals, n_cross, s->tiles);
            const uint32_t span_blocks = svo_div_up(n_spans, kThreads);
            solid_lengths_kernel<<<span_blocks, kThreads, 0, ctx->stream>>>(s->spans, n_spans, s->off, s->block_sum);
            solid_total_kernel<<<1, kTopThreads, 0, ctx->stream>>>(s->block_sum.get(), span_blocks, status);
            HIP_TRY(ctx, hipGetLastError());
            if ((rc = s->status.read(ctx))) return rc;
            count = uint64_t(st[kStCountHi]) << 32 | st[kStCountLo];
            if (count > cap) return over_cap(count, "cells");
        }
        HIP_TRY(ctx, s->timer.mark(ctx, kEvSpans));
        if (out_dev && count) {
            if (as_spans) {
                tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(runs, runs, status + kStIntervals, n_cross, s->tiles);
            } else {
                if ((rc = svo_scan_u32(ctx, s->off, n_spans))) return rc;
                solid_cells_kernel<<<svo_div_up(count, kTile), kThreads, 0, ctx->stream>>>(s->spans, s->off, n_spans, (uint32_t)count, out_dev);
            }
            HIP_TRY(ctx, hipGetLastError());
        }
    } else {
        HIP_TRY(ctx, s->timer.mark(ctx, kEvSpans));
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEmit));
    *n_out = count;
    if (n_open_out) *n_open_out = n_open;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_solid_timing(svo_ctx *ctx, float ms_out[SVO_SOLID_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->solid) return svo_fail(ctx, SVO_ERR_STATE, "no mesh voxelised solid on this context yet");
    return ctx->solid->timer.read(ctx, ms_out);
}

}  // extern "C"

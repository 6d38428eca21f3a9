// svo_scan.h -- the tiled count, scan and emit of the GPU passes: svo_proc.hip (a level's ranks), svo_build.hip (the
// level passes, the sort's digit counts), svo_adapt.hip (the expand's compactions), svo_structure.hip (sites, stamp),
// svo_voxelize.hip (a level's pairs), svo_solid.hip (a level's pairs, heads, intervals, runs), svo_surface.hip (the
// kept entries or faces), svo_surface_merge.hip (the runs of rectangles) and svo_components.hip (the roots); svo_compact.hip, svo_list.hip
// (through svo_tree_discover), svo_edit.hip and svo_adapt.hip scan an array in place with svo_scan_u32.  No atomics: an
// output's place depends on the inputs alone.
// A tile is kTile items, kPer consecutive ones per thread, so ranks follow the items' order.  A pass is three launches:
//   tile_count_kernel<Items>          a thread loads the state of its items; the block adds their counts into the tile's sum
//   tile_offsets_kernel               one block scans the tile sums in place and writes their total
//   tile_emit_kernel<Items, Emit>     the same state again; rank = the tile's offset + the block's exclusive scan of the
//                                     counts; the thread emits its items one after another from that rank on; or
//   tile_scatter_kernel<Items, Emit>  for up to 8 outputs per item, flagged in a byte: ranks in LDS, emits in rows of kThreads
// The functors travel by value as kernel arguments.  Items: load(i0, m) gives the state of the thread's items [i0, i0 +
// kPer) of the m live ones, whatever the emit needs of them (words and a kept mask, keys and flags, a uint4 of mask
// bytes), so nothing is loaded twice; count(state) what they add to the rank (a popcount of flags, a sum of values);
// for the scatter, flags(state, k) item k's flag byte.  Emit: emit(items, i0, state, rank) writes the thread's outputs
// from `rank` on, the scatter's emit(items, i, flag byte, first rank) item i's; every emit keeps its own bounds guard.
// m is m_max or, with m_dev, the device's min(*m_dev, m_max): the grid covers the host's bound, and a block wholly behind
// m returns before it touches anything.  The launches (svo_tile_count, svo_tile_pass, svo_scan_u32) stand below the
// kernels, not in svo_ctx.h, which plain C++ files include too; all in an anonymous namespace: a copy per pass file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svo_ctx.h"
#include "svo_group.h"  // (kThreads)

namespace {

constexpr uint32_t kPer = 16;                // items per thread of a tile
constexpr uint32_t kTile = kThreads * kPer;  // items per tile
constexpr uint32_t kTopThreads = 1024;       // threads of the one block that scans the tile sums
static_assert(kPer == 16, "a thread's flags are one 16-bit mask, its byte-sized items one uint4 (svo_proc.hip, svo_voxelize.hip)");
static_assert(kTile * 8 < (1u << 24), "tile_scatter_kernel packs an item's rank in the tile above its flag byte");

template <int N>
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t s[N];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const uint32_t a = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    if (total) *total = s[N - 1];
    const uint32_t r = s[t] - v;
    __syncthreads();  // (a following call reuses s)
    return r;
}

// the minimum of v over the block's N threads, in every thread
template <int N>
__device__ inline uint32_t block_min(uint32_t v) {
    __shared__ uint32_t s[N];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = N / 2; off > 0; off >>= 1) {
        if (t < off) s[t] = min(s[t], s[t + off]);
        __syncthreads();
    }
    const uint32_t r = s[0];
    __syncthreads();  // (a following call reuses s)
    return r;
}

// One block takes the minimum of the blocks' minima: out[j] = min over i < n_blocks of block_minima[C * i + j], j < C.
template <uint32_t C>
__global__ __launch_bounds__(kTopThreads) void min_of_blocks_kernel(const uint32_t *block_minima, uint32_t n_blocks, uint32_t *out) {
    for (uint32_t j = 0; j < C; j++) {
        uint32_t v = 0xFFFFFFFFu;
        for (uint32_t i = threadIdx.x; i < n_blocks; i += kTopThreads) v = min(v, block_minima[uint64_t(C) * i + j]);
        v = block_min<kTopThreads>(v);
        if (threadIdx.x == 0) out[j] = v;
    }
}

__device__ inline uint32_t input_count(const uint32_t *m_dev, uint32_t m_max) { return m_dev ? min(*m_dev, m_max) : m_max; }

template <class Items>
__global__ __launch_bounds__(kThreads) void tile_count_kernel(Items items, const uint32_t *m_dev, uint32_t m_max, uint32_t *tile_sum) {
    const uint32_t m = input_count(m_dev, m_max);
    if (blockIdx.x * kTile >= m) return;  // (the top kernel reads only the live tiles)
    uint32_t total;
    block_exclusive_scan<kThreads>(items.count(items.load(blockIdx.x * kTile + threadIdx.x * kPer, m)), &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// One block scans the tile sums in place (exclusive) and writes their total (total_out null: nowhere).  The tile count is
// n_tiles, or, with m_dev, that of the *m_dev (at most m_max) items a compaction reads.
__global__ __launch_bounds__(kTopThreads) void tile_offsets_kernel(uint32_t *tile_sum, uint32_t n_tiles, const uint32_t *m_dev,
                                                                   uint32_t m_max, uint32_t *total_out) {
    if (m_dev) n_tiles = (input_count(m_dev, m_max) + kTile - 1) / kTile;
    const uint32_t per = (n_tiles + kTopThreads - 1) / kTopThreads;
    const uint32_t lo = threadIdx.x * per, hi = min(lo + per, n_tiles);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += tile_sum[i];
    uint32_t total;
    uint32_t run = block_exclusive_scan<kTopThreads>(sum, &total);
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t v = tile_sum[i];
        tile_sum[i] = run;
        run += v;
    }
    if (threadIdx.x == 0 && total_out) *total_out = total;
}

template <class Items, class Emit>
__global__ __launch_bounds__(kThreads) void tile_emit_kernel(Items items, Emit emit, const uint32_t *m_dev, uint32_t m_max,
                                                             const uint32_t *__restrict__ tile_off) {
    const uint32_t m = input_count(m_dev, m_max), i0 = blockIdx.x * kTile + threadIdx.x * kPer;
    if (blockIdx.x * kTile >= m) return;
    const auto state = items.load(i0, m);
    emit(items, i0, state, tile_off[blockIdx.x] + block_exclusive_scan<kThreads>(items.count(state), nullptr));
}

template <class Items, class Emit>
__global__ __launch_bounds__(kThreads) void tile_scatter_kernel(Items items, Emit emit, uint32_t m, const uint32_t *__restrict__ tile_off) {
    // per item of the tile: its outputs' offset in the tile << 8 | its flag byte; one word of padding per 32, so that the
    // threads' runs of kPer words fall on different banks
    __shared__ uint32_t at[kTile + kTile / 32];
    const uint32_t tile0 = blockIdx.x * kTile;
    const auto state = items.load(tile0 + threadIdx.x * kPer, m);
    uint32_t run = block_exclusive_scan<kThreads>(items.count(state), nullptr);
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
        const uint32_t j = threadIdx.x * kPer + k, bits = items.flags(state, k) & 0xFFu;
        at[j + (j >> 5)] = run << 8 | bits;
        run += __popc(bits);
    }
    __syncthreads();
    const uint32_t base = tile_off[blockIdx.x];
    for (uint32_t row = 0; row < kPer; row++) {
        const uint32_t j = row * kThreads + threadIdx.x, i = tile0 + j;
        if (i >= m) break;
        const uint32_t mine = at[j + (j >> 5)];
        if (mine & 0xFFu) emit(items, i, mine & 0xFFu, base + (mine >> 8));
    }
}

// ---- the scatter's items whose flags are a byte array (the child masks of a level's pairs: svo_voxelize.hip, svo_solid.hip;
// the head bytes of svo_surface_merge.hip's runs, in a count and an emit) ----
// The state is the bytes of a thread's kPer consecutive items as one uint4; the array is padded to whole tiles, and what
// lies behind m is not counted.
struct FlagBytes {
    const uint8_t *mask;
    __device__ uint4 load(uint32_t i0, uint32_t m) const {
        uint4 w = *reinterpret_cast<const uint4 *>(mask + i0);
        const auto live = [&](uint32_t first) { return first >= m ? 0u : m - first >= 4 ? 0xFFFFFFFFu : (1u << 8 * (m - first)) - 1u; };
        w.x &= live(i0);
        w.y &= live(i0 + 4);
        w.z &= live(i0 + 8);
        w.w &= live(i0 + 12);
        return w;
    }
    __device__ uint32_t count(const uint4 &w) const { return __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w); }
    __device__ uint32_t flags(const uint4 &w, uint32_t k) const {
        const uint32_t q[4] = {w.x, w.y, w.z, w.w};
        return q[k / 4] >> 8 * (k % 4);
    }
};

// The sum of v[0, n) in 64 bits by the one block of kTopThreads that calls it, into out[0] (the low half) and out[1]: for
// a total that tile_offsets_kernel's 32 bits may not hold, before it is compared with a cap.
template <typename T>
__device__ inline void block_total64(const T *v, uint32_t n, uint32_t *out) {
    __shared__ uint64_t s[kTopThreads];
    uint64_t sum = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kTopThreads) sum += v[i];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = kTopThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = uint32_t(s[0]);
        out[1] = uint32_t(s[0] >> 32);
    }
}

// ---- the in-place exclusive scan of a[0, n) as such a pass: its items and its emit in one ----
struct ScanInPlace {
    uint32_t *a, n;
    struct State {
        uint32_t v[kPer];
    };
    __device__ State load(uint32_t i0, uint32_t) const {
        State s;
        for (uint32_t j = 0; j < kPer; j++) s.v[j] = i0 + j < n ? a[i0 + j] : 0u;
        return s;
    }
    __device__ uint32_t count(const State &s) const {
        uint32_t sum = 0;
        for (uint32_t v : s.v) sum += v;
        return sum;
    }
    __device__ void operator()(const ScanInPlace &, uint32_t i0, const State &s, uint32_t r) const {
        for (uint32_t j = 0; j < kPer; r += s.v[j++])
            if (i0 + j < n) a[i0 + j] = r;
    }
};

// ---- the host side, on the context's stream; n_tiles covers m_max, and the caller owns tile_sum ----
// The first two launches, for a caller that reads the total (*total_out; null: nowhere) before it launches the third;
// svo_tile_pass enqueues all three.
template <class Items>
int svo_tile_count(svo_ctx *ctx, const Items &items, uint32_t n_tiles, const uint32_t *m_dev, uint32_t m_max, uint32_t *tile_sum,
                   uint32_t *total_out) {
    tile_count_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(items, m_dev, m_max, tile_sum);
    tile_offsets_kernel<<<1, kTopThreads, 0, ctx->stream>>>(tile_sum, n_tiles, m_dev, m_max, total_out);
    HIP_TRY(ctx, hipGetLastError());
    return SVO_OK;
}
template <class Items, class Emit>
int svo_tile_pass(svo_ctx *ctx, const Items &items, const Emit &emit, uint32_t n_tiles, const uint32_t *m_dev, uint32_t m_max,
                  uint32_t *tile_sum, uint32_t *total_out) {
    if (int rc = svo_tile_count(ctx, items, n_tiles, m_dev, m_max, tile_sum, total_out)) return rc;
    tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(items, emit, m_dev, m_max, tile_sum);
    HIP_TRY(ctx, hipGetLastError());
    return SVO_OK;
}

// Exclusive scan of a[0, n) in place; the tile sums live in the context's own buffer.
inline int svo_scan_u32(svo_ctx *ctx, uint32_t *a, uint32_t n) {
    const uint32_t nt = svo_div_up(n, kTile);
    if (int rc = svo_grow(ctx, (size_t)nt, &ctx->scan_tiles)) return rc;
    return n ? svo_tile_pass(ctx, ScanInPlace{a, n}, ScanInPlace{a, n}, nt, nullptr, n, ctx->scan_tiles, nullptr) : SVO_OK;
}

}  // namespace

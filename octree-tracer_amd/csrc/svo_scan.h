// svo_scan.h -- the scan pieces of the GPU tree passes (svo_proc.hip, svo_build.hip): the tile shape, a block-wide
// exclusive scan and minimum and the one-block scan of the tile sums.  Everything sits in an anonymous namespace, so every pass file
// that includes this header compiles its own copies, as it did when each file had its own.  The other shared device
// pieces: svo_morton.h (the Morton convention), svo_mip.h (mip colours); the host ones are in svo_ctx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svo_group.h"  // (kThreads)

namespace {

constexpr uint32_t kPer = 16;                // items per thread of a tile
constexpr uint32_t kTile = kThreads * kPer;  // items per tile
constexpr uint32_t kTopThreads = 1024;       // threads of the one block that scans the tile sums

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

__device__ inline uint32_t input_count(const uint32_t *m_dev, uint32_t m_max) { return m_dev ? min(*m_dev, m_max) : m_max; }

// One block scans the tile sums in place (exclusive) and writes their total.  The tile count is n_tiles, or, with m_dev,
// that of the *m_dev (at most m_max) items a compaction reads.
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
    if (threadIdx.x == 0) *total_out = total;
}

}  // namespace

// svo_mip.h -- mip colours of chunk trees in the 8-byte <id>.bin layout, shared by the world builder
// (svo_build.hip) and the procedural world generator (svo_proc.hip).  A node is a uint2: x = pointer (interior: index of
// its child group in the chunk; leaf: >= SVO_CHUNK_OFFSET), y = r | g << 8 | b << 16.  Levels run bottom-up, one launch
// per level and one lane per node; a lane reads its child group (64 contiguous bytes) once and writes its own rgb word.
// No atomics, no scratch.  mip_of is also the host's formula for a written chunk's top_mip (chunk_top_mip in
// svo_build.hip, for svo_cpu_octree_build and svo_world_writer).  Everything sits in an anonymous namespace, like svo_scan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svo_host.h"  // SVO_CHUNK_OFFSET

namespace {

// World::generate_mip_tree's average_children (world.rs:311-328) in integers: per channel max(1, sum / count) over the
// non-(0,0,0) children, (1,1,1) when there are none.  sum <= 8 * 255 and count is 1..8, so the f32 quotient the host
// truncates is never within 1/8 of the next integer and equals the integer quotient (pinned exhaustively by
// tests/test_world_build_host.py).
__host__ __device__ inline uint32_t mip_of(const uint32_t rgb[8]) {
    uint32_t r = 0, g = 0, b = 0, count = 0;
    for (int c = 0; c < 8; c++) {
        const uint32_t v = rgb[c] & 0xFFFFFFu;
        if (!v) continue;
        r += v & 0xFFu;
        g += (v >> 8) & 0xFFu;
        b += v >> 16;
        count++;
    }
    if (!count) return 0x010101u;
    r /= count;
    g /= count;
    b /= count;
    return (r ? r : 1u) | (g ? g : 1u) << 8 | (b ? b : 1u) << 16;
}

// Node i of a chunk of n nodes (nodes: the chunk's first node).  Leaves pass through.
__device__ inline void mip_node(uint2 *nodes, uint32_t i, uint32_t n) {
    const uint32_t ptr = nodes[i].x;
    if (ptr >= SVO_CHUNK_OFFSET || ptr > n - 8u) return;  // (a pointer past the chunk cannot come from the emit)
    const uint4 *g = reinterpret_cast<const uint4 *>(nodes + ptr);
    uint32_t rgb[8];
    for (int k = 0; k < 4; k++) {
        const uint4 q = g[k];
        rgb[2 * k] = q.y;
        rgb[2 * k + 1] = q.w;
    }
    nodes[i].y = mip_of(rgb);
}

// One level of one chunk: nodes [first, first + count) of a chunk of n nodes.
__global__ __launch_bounds__(256) void mip_level_kernel(uint2 *nodes, uint32_t first, uint32_t count, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) mip_node(nodes, first + i, n);
}

}  // namespace

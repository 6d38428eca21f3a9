// svo_morton.h -- the one Morton convention of the GPU tree passes (svo_build.hip, svo_proc.hip, svo_sample.hip,
// svo_list.hip, svo_surface.hip), on the host and on the device: bit b of x, y, z sits in key bits 3b + 2, 3b + 1, 3b, so
// three key bits are a child index x*4 + y*2 + z and level 1 is in the top bits.  depth <= 21 (a key fits 63 bits).
// Everything sits in an anonymous namespace, like svo_scan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__host__ __device__ inline uint64_t morton_encode(uint32_t x, uint32_t y, uint32_t z, uint32_t depth) {
    uint64_t k = 0;
    for (uint32_t b = 0; b < depth; b++)
        k |= uint64_t((x >> b) & 1u) << (3 * b + 2) | uint64_t((y >> b) & 1u) << (3 * b + 1) | uint64_t((z >> b) & 1u) << (3 * b);
    return k;
}

// the child index of the cell (x, y, z) on the level whose bit of the coordinates is b: the key's bits 3b + 2 .. 3b
__host__ __device__ inline uint32_t morton_child(uint32_t x, uint32_t y, uint32_t z, uint32_t b) {
    return ((x >> b) & 1u) << 2 | ((y >> b) & 1u) << 1 | ((z >> b) & 1u);
}

// K: the key's own width (a kernel whose keys fit 32 bits decodes in 32-bit registers)
template <typename K>
__host__ __device__ inline void morton_decode(K k, uint32_t depth, uint32_t &x, uint32_t &y, uint32_t &z) {
    x = y = z = 0;
    for (uint32_t b = 0; b < depth; b++) {
        z |= uint32_t((k >> (3 * b)) & 1u) << b;
        y |= uint32_t((k >> (3 * b + 1)) & 1u) << b;
        x |= uint32_t((k >> (3 * b + 2)) & 1u) << b;
    }
}

// A key with a leading 1 above its 3 bits per level (the listing's prefixes, svo_list.hip): how many levels it holds,
// which is the level of the words of a group with Morton prefix `key`, or of a word with cell key `key`, minus one
__device__ inline uint32_t key_bits(uint64_t key) { return (63u - (uint32_t)__clzll((long long)key)) / 3u; }

// Dilated-integer arithmetic: one coordinate's bits stay where they are in the key, every third bit.  axis 0, 1, 2 = x, y, z.
__host__ __device__ inline uint64_t morton_axis_mask(uint32_t axis, uint32_t levels) {
    return (0x1249249249249249ull << (2u - axis)) & ((1ull << 3u * levels) - 1u);
}
// the key of the cell one step up (up != 0) or down along the axis whose bits are `mask`; the caller has checked that the
// coordinate is not at that end of the grid (all of its bits set, or none), so no carry leaves the mask
__host__ __device__ inline uint64_t morton_step(uint64_t k, uint64_t mask, bool up) {
    const uint64_t c = up ? (k | ~mask) + 1u : (k & mask) - 1u;  // the other axes' bits pass the carry on, or the borrow
    return (k & ~mask) | (c & mask);
}

}  // namespace

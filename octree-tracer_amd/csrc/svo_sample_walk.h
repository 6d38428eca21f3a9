// svo_sample_walk.h -- the sampler's rule for one cell (include/svo_hip.h) on the device, for the two files
// that ask what a cell of the `depth` grid holds: svo_sample.hip and svo_distance.hip.  Everything sits in an anonymous
// namespace, like svo_morton.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svo_hip.h"
#include "svo_morton.h"

namespace {

struct Sample {
    uint32_t value, level, index;
};

// The rule for one cell (include/svo_hip.h) from `level` on, `group` being the group of that level on the cell's path.
// Every index read is below n_words: group is 0 (n_words >= 8) or a pointer that passed the check.
__device__ inline Sample sample_walk(const uint32_t *__restrict__ words, uint64_t n_words, uint32_t x, uint32_t y, uint32_t z,
                                     uint32_t depth, uint32_t level, uint32_t group) {
    for (;; level++) {
        const uint32_t i = group + morton_child(x, y, z, depth - level);
        const uint32_t pointer = words[i] >> 4;
        if (pointer >= SVO_VOXEL_OFFSET) return {pointer - SVO_VOXEL_OFFSET, level, i};
        if (level >= depth) return {SVO_SAMPLE_FINER, level, i};
        if ((pointer & 7u) || uint64_t(pointer) + 8u > n_words) return {SVO_SAMPLE_BROKEN, level, i};
        group = pointer;
    }
}

}  // namespace

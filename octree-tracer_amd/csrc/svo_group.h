// svo_group.h -- the constants of the tree passes, and what those that walk the tree in the node buffer
// (svo_compact.hip, svo_simplify.hip, svo_list.hip) share on the device: 8 lanes per group, one word per lane, so a wave64 handles 8
// groups, a group is one 32-byte read and its interior mask is its byte of the wave's ballot.  Everything sits in an
// anonymous namespace, like svo_scan.h, which includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svo_hip.h"

namespace {

constexpr uint32_t kThreads = 256;  // per workgroup, in every tree pass
constexpr uint32_t kEmptyWord = SVO_VOXEL_OFFSET << 4;
constexpr uint64_t kMaxWords = SVO_VOXEL_OFFSET;  // 2^27: no pointer reaches further, and pointers and colours stay apart

// What the 8 lanes of a group know of it.  Every lane of the wave must get here: the mask is a ballot.
struct GroupLane {
    uint32_t word, pointer;
    bool interior;
    uint32_t mask;   // the group's interior lanes, bit c = child c
    uint32_t below;  // how many of them are below this lane
};

__device__ inline GroupLane group_lane(const uint32_t *words, const uint32_t *order, uint32_t k, uint32_t c, bool valid) {
    GroupLane g;
    g.word = valid ? words[order[k] + c] : kEmptyWord;
    g.pointer = g.word >> 4;
    g.interior = valid && g.pointer < SVO_VOXEL_OFFSET;
    const uint64_t all = __ballot(g.interior);
    g.mask = uint32_t(all >> (__lane_id() & ~7u)) & 0xFFu;
    g.below = __popc(g.mask & ((1u << c) - 1u));
    return g;
}

}  // namespace

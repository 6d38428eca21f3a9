// svo_frontier.h -- what the two top-down edits of the tree in the node buffer share, the shape edit (svo_region.hip,
// DESIGN.md 25) and the combine of two trees (svo_combine.hip): both walk the tree level by level as a frontier
// of groups of eight words, real ones in the buffer and virtual ones that a split will make, plan every write into a list
// with one entry per frontier word of every level, and commit the list with two launches.  Their plans differ (shapes
// against a cube there, a second tree's word here) and stay in their files; here are the check that no group is reached
// twice, the commit and the list's growth.  In an anonymous namespace: a copy per file, under the names they had in
// svo_region.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "svo_ctx.h"
#include "svo_group.h"  // (kThreads)

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

__host__ __device__ inline uint32_t leaf_word(uint32_t v) { return (uint32_t(SVO_VOXEL_OFFSET) + v) << 4; }

// A group reached through a pointer is reached once: the groups [0, n) of a frontier, numbered from `first_id` on, mark
// themselves in new_of (kNone: not reached yet).  A mark that is there already, from an earlier level or from another lane
// of this launch, is a second path; so is a mark that another lane of this launch overwrote, which the check finds.
// status[SVO_WALK_DUP] says so.
__global__ __launch_bounds__(kThreads) void region_mark_kernel(const uint32_t *__restrict__ gbase, const uint32_t *__restrict__ gvirt, uint32_t n,
                                                               uint32_t first_id, uint32_t cap, uint32_t *new_of, uint32_t *status) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || gvirt[k] || (gbase[k] >> 3) >= cap) return;
    if (new_of[gbase[k] >> 3] != kNone) status[SVO_WALK_DUP] = 1u;
    else new_of[gbase[k] >> 3] = first_id + k;
}
__global__ __launch_bounds__(kThreads) void region_check_kernel(const uint32_t *__restrict__ gbase, const uint32_t *__restrict__ gvirt, uint32_t n,
                                                                uint32_t first_id, uint32_t cap, const uint32_t *__restrict__ new_of,
                                                                uint32_t *status) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || gvirt[k] || (gbase[k] >> 3) >= cap) return;
    if (new_of[gbase[k] >> 3] != first_id + k) status[SVO_WALK_DUP] = 1u;
}

// The commit: the eight leaf words of every new group, one lane per word ...
__global__ __launch_bounds__(kThreads) void region_fill_kernel(uint32_t *__restrict__ words, uint32_t new_words, const uint32_t *__restrict__ list_at,
                                                               const uint32_t *__restrict__ list_word, const uint32_t *__restrict__ list_fill,
                                                               uint32_t n) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x, i = t >> 3, c = t & 7u;
    if (i >= n || list_at[i] == kNone) return;
    const uint32_t pointer = list_word[i] >> 4;
    if (pointer < SVO_VOXEL_OFFSET && uint64_t(pointer) + 8u <= new_words) words[pointer + c] = list_fill[i];  // (a split's entry)
}
// ... and then the list, one lane per entry.
__global__ __launch_bounds__(kThreads) void region_write_kernel(uint32_t *__restrict__ words, uint32_t new_words, const uint32_t *__restrict__ list_at,
                                                                const uint32_t *__restrict__ list_word, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = list_at[i];
    if (at < new_words) words[at] = list_word[i];  // (kNone is not below it)
}

// room for `want` items in a list whose first `keep` items stay, at least doubled so that the levels' growth copies little
inline int grow_list(svo_ctx *ctx, size_t want, size_t keep, svo_dev<uint32_t> *a, svo_dev<uint32_t> *b, svo_dev<uint32_t> *c) {
    if (a->size() >= want) return SVO_OK;  // (the three grow together)
    want = std::max(want, 2 * a->size());
    for (svo_dev<uint32_t> *buf : {a, b, c})
        if (int rc = svo_grow_keep(ctx, want, buf, keep)) return rc;
    return SVO_OK;
}

}  // namespace

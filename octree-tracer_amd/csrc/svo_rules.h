// svo_rules.h -- the rules every host / device comparison rests on, stated once for svo_host.cpp and svo_adapt.hip: the
// child offset, the `>=` descent step, the world walk, what a world pointer and a node word mean, and the view rule of
// an expansion.  The device passes promise the host's results bit for bit; they keep that promise by running these
// functions, not copies of them.  Plain C++17 without HIP headers (svo_host.cpp also builds under g++); under hipcc
// every function is __host__ __device__.
#pragma once
#include <cmath>
#include <cstdint>

#include "svo_hip.h"
#include "svo_host.h"

#if defined(__HIPCC__)
#define SVO_HD __host__ __device__
#else
#define SVO_HD
#endif

namespace svo_rules {

struct Vec3 {
    float x = 0, y = 0, z = 0;
};

// Octree::pos_offset (octree.rs:154-161).  The mask changes no depth of 1 .. 31, which is all an octree walk reaches on
// either side.  A world walk may run to level 64 (chunk chains, cyclic references); there a plain shift would be
// undefined, and the mask makes the offset that of depth - 32 or depth - 64 on the host as on the device.
SVO_HD inline Vec3 pos_offset(uint32_t child, uint32_t depth) {
    const float d = float(1u << (depth & 31u));
    return {(float((child >> 2) & 1u) * 2.0f - 1.0f) / d, (float((child >> 1) & 1u) * 2.0f - 1.0f) / d,
            (float(child & 1u) * 2.0f - 1.0f) / d};
}

// One step of the `>=` point location (cpu_octree.rs:48-76, octree.rs:113-141, world.rs:201-232): the child of the
// cube centred at c that holds p -- a coordinate on the centre plane goes to the upper child -- and c becomes that
// child's centre, a cube of level `depth`.
SVO_HD inline uint32_t descend(const Vec3 &p, Vec3 &c, uint32_t depth) {
    const uint32_t child = (p.x >= c.x ? 4u : 0u) | (p.y >= c.y ? 2u : 0u) | (p.z >= c.z ? 1u : 0u);
    const Vec3 o = pos_offset(child, depth);
    c.x += o.x; c.y += o.y; c.z += o.z;
    return child;
}

// node words of the device array (octree.rs:28-34)
SVO_HD constexpr bool word_is_leaf(uint32_t w) { return (w >> 4) >= SVO_VOXEL_OFFSET; }
SVO_HD constexpr uint32_t leaf_word(uint32_t rgb) { return (SVO_VOXEL_OFFSET + rgb) << 4; }

// a world node's pointer: its child group in the same chunk, a leaf, or the root group of another chunk
SVO_HD constexpr bool ptr_is_group(uint32_t ptr) { return ptr < SVO_CHUNK_OFFSET; }
SVO_HD constexpr bool ptr_is_leaf(uint32_t ptr) { return ptr == SVO_CHUNK_OFFSET; }
SVO_HD constexpr bool ptr_is_chunk(uint32_t ptr) { return ptr > SVO_CHUNK_OFFSET; }
SVO_HD constexpr uint32_t ptr_chunk_id(uint32_t ptr) { return ptr - SVO_CHUNK_OFFSET; }
// streamed chunks are dropped when the node that references them collapses; blocks stay (adaptive.rs:104-110)
SVO_HD constexpr bool chunk_is_streamed(uint32_t id) { return id >= SVO_CHUNK_OFFSET / 2; }

// Where a world walk ended: in chunk `chunk` (`in`: the policy's handle of it), on node `index` of it, a cube of level
// `depth` centred at pos.  Not ok: the walk left the resident chunks (index 0), met a pointer past its chunk (index:
// that node) or passed 64 levels (cyclic chunk references).
template <class Handle>
struct WorldAt {
    uint32_t chunk;
    Handle in;
    uint32_t index, depth;
    Vec3 pos;
    bool ok;
};

// World::find_voxel (world.rs:201-232): the `>=` walk from chunk 0, hopping into the referenced chunk's root group at a
// chunk reference, until a leaf or level max_depth (0: no limit).  The reference unwraps a missing chunk (panic); here
// ok = false.  Chunks: find(id) -> handle, resident(handle), count(handle) -> nodes, pointer(handle, index).
template <class Chunks>
SVO_HD inline auto world_walk(const Chunks &chunks, const Vec3 &p, uint32_t max_depth) -> WorldAt<decltype(chunks.find(0u))> {
    uint32_t chunk = 0, base = 0;
    Vec3 c;
    auto cur = chunks.find(0u);
    for (uint32_t depth = 1;; ++depth) {
        if (!chunks.resident(cur)) return {chunk, cur, 0, depth, c, false};
        const uint32_t at = base + descend(p, c, depth);
        if (at >= chunks.count(cur)) return {chunk, cur, at, depth, c, false};
        const uint32_t ptr = chunks.pointer(cur, at);
        if (ptr_is_leaf(ptr) || depth == max_depth) return {chunk, cur, at, depth, c, true};
        if (ptr_is_chunk(ptr)) {
            chunk = ptr_chunk_id(ptr);
            cur = chunks.find(chunk);
            base = 0;
        } else {
            base = ptr;
        }
        if (depth >= 64) return {chunk, cur, base, depth, c, false};
    }
}

// both correctly rounded
SVO_HD inline float sqrt_rn(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsqrt_rn(v);
#else
    return std::sqrt(v);
#endif
}

// The view rule of an expansion and of the generators: the cube [lo, hi] of level `level` is refined while
// 2^level * distance(cam, cube) < lod_c.  A NaN anywhere makes the comparison false: no refinement.
SVO_HD inline bool lod_refines(const float cam[3], const float lo[3], const float hi[3], uint32_t level, float lod_c) {
    float d2 = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float d = cam[k] < lo[k] ? lo[k] - cam[k] : (cam[k] > hi[k] ? cam[k] - hi[k] : 0.0f);
        d2 += d * d;
    }
    return float(1u << level) * sqrt_rn(d2) < lod_c;
}

}  // namespace svo_rules

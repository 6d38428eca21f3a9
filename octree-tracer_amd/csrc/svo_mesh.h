// svo_mesh.h -- what the two mesh voxelisers share (svo_voxelize.hip: the surface; svo_solid.hip: the
// interior): the check and the gather of one triangle's vertices on the device, and the host's wording of
// the verdict.  A bad triangle is named as t << 1 | (0: a vertex index, 1: a coordinate); the first one is the minimum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "svo_hip.h"

namespace {

constexpr uint32_t kNoBadTriangle = 0xFFFFFFFFu;

// Triangle t's nine doubled coordinates 2q + 1 into v (of a bad triangle: those of q = 0, so that every later pass runs
// on it without harm until the host has read the verdict).  Returns kNoBadTriangle or the triangle's verdict.
__device__ inline uint32_t mesh_gather_triangle(const uint32_t *__restrict__ vq, uint32_t n_vertices, const uint32_t *__restrict__ tri,
                                                uint32_t t, uint32_t depth, int32_t v[9]) {
    uint32_t q[9];
    bool index_ok = true, coord_ok = true;
    for (uint32_t j = 0; j < 3; j++) {
        const uint32_t i = tri[3ull * t + j];
        const bool ok = i < n_vertices;
        index_ok &= ok;
        for (uint32_t a = 0; a < 3; a++) {
            q[3 * j + a] = ok ? vq[3ull * i + a] : 0u;
            coord_ok &= (q[3 * j + a] >> (depth + SVO_VOX_SUBBITS)) == 0;
        }
    }
    uint32_t bad = kNoBadTriangle;
    if (!index_ok) bad = t << 1;
    else if (!coord_ok) bad = t << 1 | 1u;
    for (uint32_t k = 0; k < 9; k++) v[k] = bad == kNoBadTriangle ? int32_t(2u * q[k] + 1u) : 1;
    return bad;
}

// the message of a verdict that is not kNoBadTriangle
inline std::string mesh_bad_triangle(uint32_t bad, uint32_t depth, uint32_t n_vertices) {
    return "triangle " + std::to_string(bad >> 1) +
           (bad & 1u ? " has a coordinate outside [0, 2^(depth + 6) = " + std::to_string(1ull << (depth + SVO_VOX_SUBBITS)) + ")"
                     : " has a vertex index outside [0, n_vertices = " + std::to_string(n_vertices) + ")");
}

}  // namespace

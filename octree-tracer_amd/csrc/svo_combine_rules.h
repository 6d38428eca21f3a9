// svo_combine_rules.h -- the rule of two trees combined, as tables over (op, the scene's value empty or not, the source's
// value empty or not): what svo_combine.hip and svo_place.hip decide a word by, stated once.
// include/svo_hip.h has the rule in words.  In an anonymous namespace: a copy per file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svo_hip.h"  // (SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE)

namespace {

// f(a, b) per cell
__host__ __device__ inline uint32_t combine_value(uint32_t op, uint32_t a, uint32_t b) {
    switch (op) {
    case SVO_COMBINE_OVER: return b ? b : a;
    case SVO_COMBINE_UNDER: return a ? a : b;
    case SVO_COMBINE_PAINT: return a && b ? b : a;
    case SVO_COMBINE_CARVE: return b ? 0u : a;
    case SVO_COMBINE_KEEP: return b ? a : 0u;
    default: return b;  // SVO_COMBINE_REPLACE
    }
}
// an interior scene word against the source's leaf or constant b: f(., b) is the identity, a constant or neither; two bits
// per (op, b != 0)
enum Whole : uint32_t { kIdentity, kConstant, kOpenIt };
__host__ __device__ inline uint32_t whole_subtree(uint32_t op, bool b_set) {
    constexpr uint32_t table = kIdentity << 0 | kConstant << 2 |   // OVER: b == 0, b != 0
                               kIdentity << 4 | kOpenIt << 6 |     // UNDER
                               kIdentity << 8 | kOpenIt << 10 |    // PAINT
                               kIdentity << 12 | kConstant << 14 | // CARVE
                               kConstant << 16 | kIdentity << 18 | // KEEP
                               kConstant << 20 | kConstant << 22;  // REPLACE
    return table >> (4u * op + 2u * uint32_t(b_set)) & 3u;
}
// ... and the constant: b for OVER and REPLACE, empty for CARVE and KEEP
__host__ __device__ inline uint32_t whole_constant(uint32_t op, uint32_t b) { return op == SVO_COMBINE_OVER || op == SVO_COMBINE_REPLACE ? b : 0u; }
// a scene leaf a against an interior source word: f(a, .) is a whatever the source holds; one bit per (op, a != 0)
__host__ __device__ inline bool leaf_stays(uint32_t op, bool a_set) {
    constexpr uint32_t table = 1u << (2 * SVO_COMBINE_UNDER + 1) | 1u << (2 * SVO_COMBINE_PAINT) | 1u << (2 * SVO_COMBINE_CARVE) | 1u << (2 * SVO_COMBINE_KEEP);
    return table >> (2u * op + uint32_t(a_set)) & 1u;
}

}  // namespace

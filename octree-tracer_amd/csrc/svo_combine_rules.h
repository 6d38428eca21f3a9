// svo_combine_rules.h -- the rule of two trees combined, as tables over (op, the scene's value empty or not, the source's
// value empty or not): what svo_combine.hip, svo_place.hip and svo_transform.hip decide a word by, stated once.
// include/svo_hip.h has the rule in words.  Then what the three passes add to the frontier walk (svo_frontier.h) alike: the
// flags and the words of a refusal, and the status words and refusals of a malformed source.  In an anonymous namespace: a
// copy per file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "svo_frontier.h"
#include "svo_hip.h"  // (SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE)

namespace {

const char *const kOpNames[] = {"over", "under", "paint", "carve", "keep", "replace"};
enum Src : uint32_t { kOut, kLeaf, kNode };  // what the source has for a frontier word's cube
// a word's flags above the walk's (svo_frontier.h): at level `depth`, where a word is neither opened nor split, which tree
// is finer under the refused word; and the same in words
constexpr uint32_t kSceneFiner = 4u, kSourceFiner = 8u;
inline const char *finer_trees(uint32_t cd) {
    return (cd & kSceneFiner) && (cd & kSourceFiner) ? "the scene and the source are interior nodes" :
           (cd & kSceneFiner) ? "the scene is an interior node" : "the source is an interior node";
}

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

// The walk's hooks of a pass with a source tree: a followed source pointer is checked by the pass's emit kernel (svo_transform.hip: by its plan kernel too) as the
// discovery checks a scene's, into two status words of the pass's own, which are tested behind the walk's.
enum { kStSrcAlign = kStWords, kStSrcRange };
struct SourcePass : FrontierPass {
    static constexpr bool kWantsCode = true;
    uint64_t src_words = 0;
    int check(svo_ctx *ctx, const uint32_t *st, uint32_t level) {
        const std::string where = "malformed source: an interior pointer at level " + std::to_string(level);
        if (st[kStSrcAlign]) return svo_fail(ctx, SVO_ERR_STATE, where + " is not a multiple of 8");
        if (st[kStSrcRange]) return svo_fail(ctx, SVO_ERR_STATE, where + " leaves the first src_words = " + std::to_string(src_words) + " words");
        return SVO_OK;
    }
};

}  // namespace

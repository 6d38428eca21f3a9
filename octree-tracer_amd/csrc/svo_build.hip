// svo_build.hip -- render-ready trees built on the GPU from a voxel list or a dense colour grid.  The
// same idea as the procedural generator (svo_proc.hip): the tree is the canonical breadth-first form of the union of
// the voxels' root-to-leaf paths, built with scans and without atomics, so the words do not depend on the run or on the
// order of distinct input voxels.
//
//   keys     one lane per voxel: Morton key (3 * depth bits, level 1 in the top bits) and payload = input index; a
//            coordinate outside [0, 2^depth) sets the error word
//   sort     stable LSD radix sort, 8-bit digits: per-tile digit counts, one scan of the counts, a stable scatter that
//            ranks a tile's items with wave64 ballots.  Stability keeps equal keys in input order
//   levels   per level a flag on the LAST element of every run of equal keys, a scan of the flags and a compaction to
//            the next level up, as one tile pass of svo_scan.h (Level<M>, LevelEmit<M>).  The first pass (leaf
//            level) keeps the last voxel of a run of equal cells: repeated put(), last one wins.  The counts of all
//            levels are read back in one copy and checked against the cap before anything is written
//   emit     the level passes again, top level last, now also writing every node's slot,
//            base_L + 8 * parent_rank + (key & 7), into the node buffer filled with the empty word
//
// An element's parent rank is the exclusive scan of the parent-level flags at that element: every run before its own has
// its flag (its last element) in front of it.  The dense grid skips keys and sort: lanes walk the cells in Morton order
// and the flag is "cell non-zero", which yields the leaf level already sorted and unique.
//
// Chunk trees (svo_cpu_octree_build, svo_world_build) take the same keys, sort and level passes in kChunk
// mode: the counting passes also find every chunk's run in each level's sorted keys, and the emit writes 8-byte <id>.bin
// nodes per chunk, which the shared mip pass (svo_mip.h) colours bottom-up before they are staged chunk by chunk.
//
// The list entry points share one front end (check_list, list_leaves: keys, sort, leaf pass), level_bounds and
// read_counts.  Shared with the other passes: the tile pass and svo_scan_u32 (svo_scan.h), the Morton convention
// (svo_morton.h), mip_of and the mip pass (svo_mip.h), svo_grow (svo_ctx.h).  This file also holds what the others borrow:
// svo_build_sort_u32 (svo_adapt.hip), svo_build_list_leaves (svo_edit.hip) and svo_world_writer, the one place that lays
// out a generated world's directory (svo_world_build here, svo_world_generate in svo_proc.hip).
#include <hip/hip_runtime.h>

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_mip.h"     // (chunk trees: the mip pass svo_proc.hip shares)
#include "svo_morton.h"  // (keys, the dense grid's cell order, chunk indices)
#include "svo_scan.h"    // (tiles of kTile items: sort, scans and compactions alike)

namespace {

constexpr int kErrSlot = 24;                      // counts[0..21]: nodes per level; counts[24]: range error
constexpr int kCountSlots = 32;

enum Mode { kDedupe = 0, kParent = 1, kDense = 2, kChunk = 3 };  // kChunk: kParent whose emit writes chunk trees

// ---- keys ----
__global__ __launch_bounds__(kThreads) void build_keys_kernel(const uint32_t *xyz, uint32_t n, uint32_t depth, uint64_t *keys,
                                                              uint32_t *vals, uint32_t *err) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = xyz[3 * size_t(i)], y = xyz[3 * size_t(i) + 1], z = xyz[3 * size_t(i) + 2];
    if ((x | y | z) >> depth) *err = 1u;  // (every writer stores the same value)
    keys[i] = morton_encode(x, y, z, depth);
    vals[i] = i;
}

// ---- sort ----
// Lanes of the wave whose digit equals this lane's, among `valid` (8 ballots, one per digit bit).
__device__ inline uint64_t match_digit(uint32_t d, uint64_t valid) {
    uint64_t peers = valid;
    for (int b = 0; b < 8; b++) {
        const uint64_t bal = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? bal : ~bal;
    }
    return peers;
}

__device__ inline uint64_t lanes_below() {
    const uint32_t lane = __lane_id();
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// Tile t's count of every digit at hist[digit * n_tiles + t], so that one exclusive scan of hist gives every (digit, tile)
// its first output position.  Counted per wave with ballots into wave-private LDS rows: no atomics.
__global__ __launch_bounds__(kThreads) void build_hist_kernel(const uint64_t *keys, uint32_t n, uint32_t shift, uint32_t *hist,
                                                              uint32_t n_tiles) {
    __shared__ uint32_t cnt[kThreads / 64][256];
    const uint32_t w = threadIdx.x / 64;
    for (uint32_t r = 0; r < kThreads / 64; r++) cnt[r][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kTile;
    for (uint32_t r = 0; r < kPer; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const bool v = i < n;
        const uint32_t d = v ? uint32_t(keys[i] >> shift) & 0xFFu : 0u;
        const uint64_t peers = match_digit(d, __ballot(v));
        if (v && (peers & lanes_below()) == 0) cnt[w][d] += __popcll(peers);  // the group's lowest lane
    }
    __syncthreads();
    uint32_t s = 0;
    for (uint32_t r = 0; r < kThreads / 64; r++) s += cnt[r][threadIdx.x];
    hist[threadIdx.x * n_tiles + blockIdx.x] = s;
}

// Stable scatter of one tile: item i of round r is tile item r * 256 + threadIdx.x, so rounds, waves and lanes walk the
// tile in input order.  An item goes to run[d] (where digit d's next item of this tile goes) + the counts of d in the
// waves before its own in this round + its rank among its wave's lanes with digit d.
__global__ __launch_bounds__(kThreads) void build_scatter_kernel(const uint64_t *keys_in, const uint32_t *vals_in, uint32_t n,
                                                                 uint32_t shift, const uint32_t *hist, uint32_t n_tiles,
                                                                 uint64_t *keys_out, uint32_t *vals_out) {
    __shared__ uint32_t run[256];
    __shared__ uint32_t cnt[kThreads / 64][256];
    const uint32_t w = threadIdx.x / 64;
    run[threadIdx.x] = hist[threadIdx.x * n_tiles + blockIdx.x];
    for (uint32_t r = 0; r < kThreads / 64; r++) cnt[r][threadIdx.x] = 0;
    const uint32_t base = blockIdx.x * kTile;
    uint64_t k[kPer];
    uint32_t v[kPer];
    for (uint32_t r = 0; r < kPer; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        k[r] = i < n ? keys_in[i] : 0ull;
        v[r] = i < n ? vals_in[i] : 0u;
    }
    __syncthreads();
    for (uint32_t r = 0; r < kPer; r++) {
        const bool valid = base + r * kThreads + threadIdx.x < n;
        const uint32_t d = uint32_t(k[r] >> shift) & 0xFFu;
        const uint64_t peers = match_digit(d, __ballot(valid));
        const uint32_t below = __popcll(peers & lanes_below());
        if (valid && below == 0) cnt[w][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + below;
            for (uint32_t q = 0; q < w; q++) pos += cnt[q][d];
            if (pos < n) {  // (always: the counts and the scatter walk the same tile)
                keys_out[pos] = k[r];
                vals_out[pos] = v[r];
            }
        }
        __syncthreads();
        uint32_t s = 0;
        for (uint32_t q = 0; q < kThreads / 64; q++) {
            s += cnt[q][threadIdx.x];
            cnt[q][threadIdx.x] = 0;
        }
        run[threadIdx.x] += s;
        __syncthreads();
    }
}

// ---- levels: flags, scans, compaction, emit ----
struct LevelIn {
    const uint64_t *keys;     // kDedupe: sorted keys; kParent: this level's unique keys
    const uint32_t *vals;     // kDedupe: input index of each key; kParent: leaf colours (last level only) or null
    const uint32_t *colours;  // kDedupe: the caller's colours or null; kDense: the grid
    uint32_t colour;          // kDedupe without colours
    const uint32_t *m_dev;    // number of input items on the device (null: m_max)
    uint32_t m_max;           // host bound of that number (the input buffer's size)
    uint32_t depth;           // kDense: grid depth
};

struct LevelOut {
    uint64_t *keys;     // compacted keys, one per run
    uint32_t *colours;  // kDedupe / kDense: the leaf colour of each
    uint32_t *index;    // kDedupe: the input index of each (null: not kept)
    uint32_t cap;       // room in keys / colours
    // emit (kParent only; words null: counting pass)
    uint32_t *words;
    uint32_t base;       // first word of this level
    uint32_t base_next;  // first word of the level below (interior nodes point there)
    uint32_t last;       // this is the leaf level
    uint32_t n_words;
    // chunk emit (kChunk only; nodes null: counting pass).  Chunk c = key >> cshift owns the nodes from coff[c] on; its
    // local level bases are cbase[c * stride + L]; start_up / start_here: the first index of chunk c in the level above /
    // this level's unique keys
    uint2 *nodes;
    uint64_t n_nodes;
    const uint64_t *coff;
    const uint32_t *cbase, *start_up, *start_here;
    uint32_t cshift, level, stride;  // level: this level's chunk-local number L
};

// A thread's 16 consecutive items of the m live ones: their keys and flags (bit j: item i0 + j ends a run / is kept).
struct LevelItems {
    uint64_t k[kPer];
    uint32_t f, m;
};

// The tile pass's items (svo_scan.h) of a level in mode M.
template <int M>
struct Level {
    LevelIn in;
    __device__ LevelItems load(uint32_t i0, uint32_t m) const {
        LevelItems s;
        s.f = 0;
        s.m = m;
        if (M == kDense) {
            const uint32_t side = 1u << in.depth;
            for (uint32_t j = 0; j < kPer; j++) {
                const uint32_t i = i0 + j;
                s.k[j] = 0;
                if (i >= m) continue;
                uint32_t x, y, z;
                morton_decode(i, in.depth, x, y, z);
                const uint32_t c = in.colours[(size_t(x) * side + y) * side + z];
                s.k[j] = i | uint64_t(c) << 32;  // (the cell's value rides in the high half)
                if (c) s.f |= 1u << j;
            }
            return s;
        }
        const uint32_t shift = M == kParent || M == kChunk ? 3u : 0u;
        for (uint32_t j = 0; j < kPer; j++) s.k[j] = i0 + j < m ? in.keys[i0 + j] : 0ull;
        const uint64_t after = i0 + kPer < m ? in.keys[i0 + kPer] : 0ull;
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t i = i0 + j;
            if (i >= m) break;
            const bool end = i + 1 == m || (s.k[j] >> shift) != ((j + 1 < kPer ? s.k[j + 1] : after) >> shift);
            s.f |= uint32_t(end) << j;
        }
        return s;
    }
    __device__ uint32_t count(const LevelItems &s) const { return __popc(s.f); }
};

// Its emit: the compaction of the flagged items to the next level up and, in an emitting pass, every item's node.
template <int M>
struct LevelEmit {
    LevelOut out;
    __device__ void operator()(const Level<M> &level, uint32_t i0, const LevelItems &s, uint32_t r) const {
        const LevelIn &in = level.in;
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t i = i0 + j;
            if (i >= s.m) break;
            if (M == kParent && out.words) {  // node i of this level: its parent's rank is r
                const uint32_t dst = out.base + 8u * r + uint32_t(s.k[j] & 7u);
                const uint32_t word = out.last ? (SVO_VOXEL_OFFSET + (in.vals[i] & 0xFFFFFFu)) << 4 : (out.base_next + 8u * i) << 4;
                if (dst < out.n_words) out.words[dst] = word;  // (always: the counts and the ranks come from the same flags)
            }
            if (M == kChunk && out.nodes) {  // node i of this level, in chunk c: its parent's rank within the chunk is r - start_up[c]
                const uint32_t c = uint32_t(s.k[j] >> out.cshift);
                const uint32_t *b = out.cbase + size_t(c) * out.stride;
                const uint64_t dst = out.coff[c] + b[out.level] + 8u * (r - out.start_up[c]) + uint32_t(s.k[j] & 7u);
                uint2 node;
                if (out.last) {  // leaf: SVO_CHUNK_OFFSET, r g b of 0x00RRGGBB (Rgb::cpu_value)
                    const uint32_t v = in.vals[i];
                    node = make_uint2(SVO_CHUNK_OFFSET, (v >> 16 & 0xFFu) | (v & 0xFF00u) | (v & 0xFFu) << 16);
                } else {  // interior: its child group, behind this level in the chunk; rgb comes from the mip pass
                    node = make_uint2(b[out.level + 1] + 8u * (i - out.start_here[c]), 0u);
                }
                if (dst < out.n_nodes) out.nodes[dst] = node;  // (always, as above)
            }
            if ((s.f >> j) & 1u) {
                if (r < out.cap) {
                    out.keys[r] = M == kParent || M == kChunk ? s.k[j] >> 3 : (M == kDense ? s.k[j] & 0xFFFFFFFFu : s.k[j]);
                    if (M == kDedupe) out.colours[r] = (in.colours ? in.colours[in.vals[i]] : in.colour) & 0xFFFFFFu;
                    if (M == kDedupe && out.index) out.index[r] = in.vals[i];
                    if (M == kDense) out.colours[r] = uint32_t(s.k[j] >> 32) & 0xFFFFFFu;
                }
                r++;
            }
        }
    }
};

// ---- chunk trees ----
// The runs of a level's sorted unique keys per chunk (c = key >> shift < n_chunks): start[c] = the first index of chunk c,
// start[n_chunks] = m.  Lane i writes the starts of the chunks from the previous key's chunk (exclusive) to its own
// (inclusive), the last lane those behind it: every entry is written once, without atomics.
__global__ __launch_bounds__(kThreads) void build_runs_kernel(const uint64_t *keys, const uint32_t *m_dev, uint32_t m_max,
                                                              uint32_t shift, uint32_t n_chunks, uint32_t *start) {
    const uint32_t m = input_count(m_dev, m_max);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint32_t c = min(uint32_t(keys[i] >> shift), n_chunks - 1);
    const uint32_t from = i ? min(uint32_t(keys[i - 1] >> shift), n_chunks - 1) + 1 : 0u;
    for (uint32_t cc = from; cc <= c; cc++) start[cc] = i;
    if (i + 1 == m)
        for (uint32_t cc = c + 1; cc <= n_chunks; cc++) start[cc] = m;
}

// One level of every chunk: lane j is slot j of the level's groups, in chunk order (8 * start_up[c] is chunk c's first
// slot); its node is cbase[c * stride + level] + the slot's offset in the chunk.
__global__ __launch_bounds__(kThreads) void build_mip_kernel(uint2 *nodes, const uint64_t *coff, const uint32_t *cbase,
                                                             const uint32_t *start_up, uint32_t n_chunks, uint32_t stride,
                                                             uint32_t level, uint32_t n_lanes) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n_lanes) return;
    const uint32_t p = j >> 3;
    uint32_t lo = 0, hi = n_chunks;  // the chunk c with start_up[c] <= p < start_up[c + 1]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start_up[mid] <= p) lo = mid;
        else hi = mid;
    }
    const uint32_t *b = cbase + size_t(lo) * stride;
    mip_node(nodes + coff[lo], b[level] + (j - 8u * start_up[lo]), b[stride - 1]);
}

__global__ __launch_bounds__(kThreads) void build_fill_kernel(uint2 *nodes, uint64_t n) {
    for (uint64_t i = blockIdx.x * uint64_t(kThreads) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kThreads)
        nodes[i] = make_uint2(SVO_CHUNK_OFFSET, 0u);
}

// The events of a build and the two timing ledgers read from them: slot k of a ledger is the time from its first event to
// its last (include/svo_hip.h: SVO_BUILD_TIMES, SVO_WORLD_BUILD_TIMES; the remaining slots are host wall times).
enum Ev { kEvStart, kEvKeys, kEvSort, kEvLevels, kEvCounts, kEvEmit, kEvEmitEnd, kEvChunkEmit, kEvChunkEmitEnd, kEvChunkMips, kEvs };
struct Slot {
    Ev first, last;
};
constexpr Slot kBuildSlots[5] = {{kEvStart, kEvKeys}, {kEvKeys, kEvSort}, {kEvSort, kEvLevels}, {kEvLevels, kEvCounts}, {kEvEmit, kEvEmitEnd}};
constexpr Slot kChunkSlots[6] = {{kEvStart, kEvKeys},    {kEvKeys, kEvSort},           {kEvSort, kEvLevels},
                                 {kEvLevels, kEvCounts}, {kEvChunkEmit, kEvChunkEmitEnd}, {kEvChunkEmitEnd, kEvChunkMips}};

}  // namespace

// Per-context workspace of the builder (svo_ctx::build): O(items), grown when a larger input comes, freed with the
// context.  keys[0] / keys[1] and vals[0] / vals[1] are the sort's ping-pong buffers, later the level passes'
// (keys[0], keys[1] by turns); keys[2] / leaf_colours hold the leaf level from the level pass to the emit.
struct svo_build_state {
    svo_dev<uint64_t> keys[3];
    svo_dev<uint32_t> vals[2];
    svo_dev<uint32_t> leaf_colours;
    size_t items() const { return leaf_colours.size(); }  // room in every one of them (the last one allocated)
    svo_dev<uint32_t> hist;   // the sort's digit counts, 256 per tile
    svo_dev<uint32_t> tiles;  // tile sums / offsets of a level pass
    svo_mirrored<> counts;      // kCountSlots words: unique nodes per level, error word
    svo_pass_timer<kEvs, SVO_BUILD_TIMES> timer;  // (spans: kBuildSlots, the sort's only when the last build sorted)
    // chunk trees (svo_world_build, svo_cpu_octree_build)
    svo_dev<uint32_t> runs;  // per level 0..21: n_chunks + 1 chunk starts, and their pinned mirror
    svo_pinned<uint32_t> runs_host;
    svo_dev<uint32_t> cbase;  // per chunk: chunk-local level bases 1 .. chunk_depth + 1 (the last = its node count)
    svo_dev<uint64_t> coff;   // per chunk: its first node in `nodes`
    svo_dev<uint2> nodes;     // every chunk's nodes, one chunk after another
    svo_pinned<void> stage;   // one chunk's bytes on their way to a file or a CpuOctree
    float cms[SVO_WORLD_BUILD_TIMES] = {};

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return counts.alloc(ctx, kCountSlots);
    }
};

namespace {

// workspace for `items` keys (and the tile sums of level passes over at most `scan_items` items)
int ensure_state(svo_ctx *ctx, size_t items, size_t scan_items, size_t hist_items) {
    int rc = svo_workspace_ensure(ctx, ctx->build);
    if (rc) return rc;
    svo_build_state *s = ctx->build.get();
    rc = svo_grow(ctx, items, &s->keys[0], &s->keys[1], &s->keys[2], &s->vals[0], &s->vals[1], &s->leaf_colours);
    if (!rc) rc = svo_grow(ctx, hist_items, &s->hist);
    if (!rc) rc = svo_grow(ctx, (size_t)svo_div_up(scan_items, kTile) + 1, &s->tiles);
    return rc;
}

// `passes` stable 8-bit radix passes over the n items in keys[0] / vals[0], which take turns with keys[1] / vals[1]; the
// result is in keys[passes & 1] / vals[passes & 1].  The digit counts are the builder's (hist: 256 per tile).
int sort_passes(svo_ctx *ctx, uint32_t n, uint32_t passes, uint64_t *const keys[2], uint32_t *const vals[2]) {
    svo_build_state *s = ctx->build.get();
    const uint32_t nt = svo_div_up(n, kTile);
    for (uint32_t k = 0; k < passes; k++) {
        const uint32_t a = k & 1;
        build_hist_kernel<<<nt, kThreads, 0, ctx->stream>>>(keys[a], n, 8 * k, s->hist, nt);
        HIP_TRY(ctx, hipGetLastError());
        int rc = svo_scan_u32(ctx, s->hist, 256 * nt);
        if (rc) return rc;
        build_scatter_kernel<<<nt, kThreads, 0, ctx->stream>>>(keys[a], vals[a], n, 8 * k, s->hist, nt, keys[a ^ 1], vals[a ^ 1]);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SVO_OK;
}
// the builder's own buffers
int sort_passes(svo_ctx *ctx, uint32_t n, uint32_t passes) {
    svo_build_state *s = ctx->build.get();
    uint64_t *const keys[2] = {s->keys[0], s->keys[1]};
    uint32_t *const vals[2] = {s->vals[0], s->vals[1]};
    return sort_passes(ctx, n, passes, keys, vals);
}

// One level pass: flags, tile counts, scan (the total goes to *total), compaction (and, with out.words or out.nodes, emit).
// `bound` is the host's bound of the input count: the grid covers it.
template <int M>
int level_pass(svo_ctx *ctx, const LevelIn &in, const LevelOut &out, uint64_t bound, uint32_t *total) {
    svo_build_state *s = ctx->build.get();
    const uint32_t nt = std::max(svo_div_up(bound, kTile), 1u);
    return svo_tile_pass(ctx, Level<M>{in}, LevelEmit<M>{out}, nt, in.m_dev, in.m_max, s->tiles, total);
}

// A chunked build: chunk c of level L's keys is key >> 3 * (L - world_depth).  Counting passes (nodes null)
// also write the chunk runs of levels world_depth .. depth - 1 into runs; the emit writes chunk trees into nodes.
struct ChunkPlan {
    uint32_t world_depth, n_chunks;
    uint2 *nodes;
    uint64_t n_nodes;
};

// The parent passes L = depth .. stop over the leaf level in keys[2] / leaf_colours: level L's unique keys in, level
// L-1's out (keys[0] and keys[1] by turns), m_{L-1} into counts[L-1].  With words: the emit, level L's slots too.
int parent_passes(svo_ctx *ctx, uint32_t depth, uint32_t stop, const uint64_t *bound, uint32_t *words, const uint64_t *base,
                  uint64_t n_words, const ChunkPlan *plan = nullptr) {
    svo_build_state *s = ctx->build.get();
    const uint64_t *src = s->keys[2];
    for (uint32_t l = depth, turn = 0; l >= stop; l--, turn ^= 1) {
        LevelIn in{};
        in.keys = src;
        in.vals = l == depth ? s->leaf_colours : nullptr;
        in.m_dev = s->counts.dev + l;
        in.m_max = (uint32_t)s->items();
        LevelOut out{};
        out.keys = s->keys[turn];
        out.cap = (uint32_t)s->items();
        out.words = words;
        if (words) {
            out.base = (uint32_t)base[l];
            out.base_next = l < depth ? (uint32_t)base[l + 1] : 0u;
            out.last = l == depth;
            out.n_words = (uint32_t)n_words;
        }
        int rc;
        if (plan) {
            const uint32_t wd = plan->world_depth, row = plan->n_chunks + 1;
            if (!plan->nodes && l < depth && l >= wd) {
                build_runs_kernel<<<std::max(svo_div_up(bound[l], kThreads), 1u), kThreads, 0, ctx->stream>>>(
                    src, s->counts.dev + l, in.m_max, 3 * (l - wd), plan->n_chunks, s->runs + size_t(l) * row);
                HIP_TRY(ctx, hipGetLastError());
            }
            if (plan->nodes) {
                out.nodes = plan->nodes;
                out.n_nodes = plan->n_nodes;
                out.coff = s->coff;
                out.cbase = s->cbase;
                out.start_up = s->runs + size_t(l - 1) * row;
                out.start_here = s->runs + size_t(l) * row;
                out.cshift = 3 * (l - wd);
                out.level = l - wd;
                out.stride = depth - wd + 2;
                out.last = l == depth;
            }
            rc = level_pass<kChunk>(ctx, in, out, bound[l], s->counts.dev + l - 1);
        } else {
            rc = level_pass<kParent>(ctx, in, out, bound[l], s->counts.dev + l - 1);
        }
        if (rc) return rc;
        src = s->keys[turn];
    }
    return SVO_OK;
}

// The parameters every build has; `depth` is null when the caller passed no params.
int check_depth(svo_ctx *ctx, const uint32_t *depth, uint32_t max_depth) {
    if (!depth) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    return svo_check_depth(ctx, *depth, max_depth);
}

// The three list entry points: svo_nodes_build (chunked null), svo_cpu_octree_build (a single tree) and svo_world_build.
int check_list(svo_ctx *ctx, const uint32_t *depth, const svo_chunk_build_params *chunked, bool world, const uint32_t *xyz, size_t n) {
    int rc = check_depth(ctx, depth, 21);
    if (rc) return rc;
    if (chunked && !world && chunked->world_depth != 0) return svo_fail(ctx, SVO_ERR_ARG, "world_depth must be 0 for a single tree");
    if (chunked && world && (chunked->world_depth < 1 || chunked->world_depth > 4 || chunked->world_depth >= *depth))
        return svo_fail(ctx, SVO_ERR_ARG, "world_depth must be 1..4 and below depth (got " + std::to_string(chunked->world_depth) +
                                              ", depth " + std::to_string(*depth) + ")");
    if (n >= (1ull << 31)) return svo_fail(ctx, SVO_ERR_ARG, "at most 2^31 - 1 voxels per build");
    if (!xyz && n) return svo_fail(ctx, SVO_ERR_ARG, "null coordinates");
    return SVO_OK;
}

uint64_t word_limit(const svo_ctx *ctx, const svo_build_params *p) {
    uint64_t lim = std::min<uint64_t>(ctx->capacity, kMaxWords);
    return p->max_words ? std::min<uint64_t>(lim, p->max_words) : lim;
}

// The front end of the list entry points: workspace for n voxels (chunked: and for runs_items chunk starts, cleared with
// the counts), keys, sort, and the leaf pass, which keeps the last voxel of every run of equal keys in keys[2] /
// leaf_colours and their number in counts[depth]; with keep_index also their input indices, in the sort's spare vals buffer.
int list_leaves(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, uint32_t depth, uint32_t default_colour,
                size_t runs_items, bool keep_index = false) {
    const uint32_t nt = svo_div_up(n, kTile);
    int rc = ensure_state(ctx, n, n, 256ull * nt);
    if (rc) return rc;
    svo_build_state *s = ctx->build.get();
    if ((rc = svo_grow(ctx, runs_items, &s->runs))) return rc;
    if ((rc = svo_grow_pinned(ctx, runs_items, &s->runs_host))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    HIP_TRY(ctx, s->counts.zero(ctx));
    if (runs_items) HIP_TRY(ctx, hipMemsetAsync(s->runs, 0, runs_items * sizeof(uint32_t), ctx->stream));
    build_keys_kernel<<<svo_div_up(n, kThreads), kThreads, 0, ctx->stream>>>(xyz, (uint32_t)n, depth, s->keys[0], s->vals[0],
                                                                             s->counts.dev + kErrSlot);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, kEvKeys));
    const uint32_t passes = (3 * depth + 7) / 8;
    if ((rc = sort_passes(ctx, (uint32_t)n, passes))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvSort));
    LevelIn in{};
    in.keys = s->keys[passes & 1];
    in.vals = s->vals[passes & 1];
    in.colours = colours;
    in.colour = default_colour;
    in.m_max = (uint32_t)n;
    LevelOut out{};
    out.keys = s->keys[2];
    out.colours = s->leaf_colours;
    out.index = keep_index ? s->vals[(passes & 1) ^ 1] : nullptr;
    out.cap = (uint32_t)s->items();
    return level_pass<kDedupe>(ctx, in, out, n, s->counts.dev + depth);
}

// Host bounds of the unique nodes per level, from the leaf level's: m_L <= m_{L+1} and m_L <= 8^L.
void level_bounds(uint64_t bound[23], uint32_t depth, uint64_t leaf_bound) {
    bound[depth] = leaf_bound;
    for (uint32_t l = depth; l-- > 0;) bound[l] = std::min<uint64_t>(bound[l + 1], 1ull << (3 * l));
}

// The one read-back between the counting passes and the emit: the counts of all levels (and, chunked, the chunk starts)
// into their pinned mirrors; fails on the keys kernel's range error word.
int read_counts(svo_ctx *ctx, uint32_t depth, size_t runs_items) {
    svo_build_state *s = ctx->build.get();
    HIP_TRY(ctx, s->timer.mark(ctx, kEvLevels));
    HIP_TRY(ctx, s->counts.copy(ctx));
    if (runs_items) HIP_TRY(ctx, hipMemcpyAsync(s->runs_host, s->runs, runs_items * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvCounts));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (s->counts.host()[kErrSlot])
        return svo_fail(ctx, SVO_ERR_ARG, "a voxel coordinate is outside [0, 2^depth) (depth " + std::to_string(depth) + ")");
    return SVO_OK;
}

// Both word-tree entry points after their leaf pass: the other level passes, the read-back of the counts, the cap, the emit.
int finish(svo_ctx *ctx, const svo_build_params *p, uint64_t leaf_bound, double t0, bool sorted, uint64_t *n_words_out) {
    svo_build_state *s = ctx->build.get();
    const uint32_t depth = p->depth;
    uint64_t bound[23] = {};
    level_bounds(bound, depth, std::min<uint64_t>(leaf_bound, s->items()));
    int rc = parent_passes(ctx, depth, 2, bound, nullptr, nullptr, 0);
    if (rc) return rc;
    if ((rc = read_counts(ctx, depth, 0))) return rc;
    const uint32_t *m = s->counts.host();
    const uint64_t limit = word_limit(ctx, p);
    if (m[depth] > s->items())  // (dense: more solid cells than the cap has words)
        return svo_fail(ctx, SVO_ERR_CAP, std::to_string(m[depth]) + " leaves cannot fit in " + std::to_string(limit) + " words");
    // breadth-first bases: level 1 (the root group) at 0, level L+1 behind level L's 8 * m_{L-1} words
    uint64_t base[23] = {0, 0};
    for (uint32_t l = 1; l < depth; l++) base[l + 1] = base[l] + 8ull * (l == 1 ? 1u : m[l - 1]);
    const uint64_t n_words = base[depth] + 8ull * (depth == 1 ? 1u : m[depth - 1]);
    if (n_words > limit)
        return svo_fail(ctx, SVO_ERR_CAP, "the tree needs " + std::to_string(n_words) + " words, over the limit of " +
                                              std::to_string(limit) + " (max_words, the node buffer's capacity, 2^27)");
    for (uint32_t l = 1; l <= depth; l++) bound[l] = m[l];
    // emit: behind every earlier write to the store, whichever context issued it
    rc = svo_store_order_after_write(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEmit));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->nodes, (int)kEmptyWord, n_words, ctx->stream));
    rc = parent_passes(ctx, depth, 1, bound, ctx->nodes, base, n_words);
    if (rc) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEmitEnd));
    rc = svo_store_note_write(ctx);
    if (rc) return rc;
    *n_words_out = n_words;
    for (int k = 0; k < 5; k++) {  // (dense: no sort)
        const bool none = k == 1 && !sorted;
        s->timer.span[k][0] = none ? nullptr : s->timer.ev[kBuildSlots[k].first];
        s->timer.span[k][1] = none ? nullptr : s->timer.ev[kBuildSlots[k].last];
    }
    s->timer.finish(t0);
    return SVO_OK;
}

// n == 0 (CpuOctree::new(0)): the root group of 8 empty words.
int build_empty(svo_ctx *ctx, const svo_build_params *p, uint64_t *n_words_out) {
    if (word_limit(ctx, p) < 8) return svo_fail(ctx, SVO_ERR_CAP, "the empty tree needs 8 words, over max_words");
    int rc = svo_store_order_after_write(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->nodes, (int)kEmptyWord, 8, ctx->stream));
    rc = svo_store_note_write(ctx);
    if (rc) return rc;
    if (ctx->build) ctx->build->timer.none();
    *n_words_out = 8;
    return SVO_OK;
}

__global__ __launch_bounds__(kThreads) void build_widen_kernel(const uint32_t *in, uint32_t n, uint64_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    keys[i] = in[i];
    vals[i] = i;
}

__global__ __launch_bounds__(kThreads) void build_narrow_kernel(const uint64_t *keys, uint32_t n, uint32_t *out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = (uint32_t)keys[i];
}

}  // namespace

// The radix sort above, for other passes on the ctx stream (svo_adapt.hip sorts its node lists with it).
int svo_build_sort_u32(svo_ctx *ctx, const uint32_t *in, uint32_t n, uint32_t *out) {
    if (!n) return SVO_OK;
    const uint32_t nt = svo_div_up(n, kTile), grid = svo_div_up(n, kThreads);
    int rc = ensure_state(ctx, n, 0, 256ull * nt);
    if (rc) return rc;
    svo_build_state *s = ctx->build.get();
    build_widen_kernel<<<grid, kThreads, 0, ctx->stream>>>(in, n, s->keys[0], s->vals[0]);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = sort_passes(ctx, n, 4))) return rc;  // (4 passes of 8 bits: the result is back in keys[0])
    build_narrow_kernel<<<grid, kThreads, 0, ctx->stream>>>(s->keys[0], n, out);
    HIP_TRY(ctx, hipGetLastError());
    return SVO_OK;
}

// The same sort of n (key, value) pairs by the keys' low `bits` bits, in place, for other passes on the ctx stream
// (svo_solid.hip sorts its crossings with it): ceil(bits / 8) passes between the caller's arrays and the builder's
// keys[1] / vals[1].  Nothing is copied back: *keys_dev and *vals_dev come back pointing at the sorted arrays, the
// caller's own after an even number of passes, the builder's after an odd one; those have room for n + 1 items and hold
// until the next call that uses the builder's workspace.
int svo_build_sort_u64(svo_ctx *ctx, uint64_t **keys_dev, uint32_t **vals_dev, uint32_t n, uint32_t bits) {
    if (!n) return SVO_OK;
    int rc = ensure_state(ctx, (size_t)n + 1, 0, 256ull * svo_div_up(n, kTile));
    if (rc) return rc;
    svo_build_state *s = ctx->build.get();
    const uint32_t passes = (bits + 7) / 8;
    uint64_t *const keys[2] = {*keys_dev, s->keys[1]};
    uint32_t *const vals[2] = {*vals_dev, s->vals[1]};
    if ((rc = sort_passes(ctx, n, passes, keys, vals))) return rc;
    *keys_dev = keys[passes & 1];
    *vals_dev = vals[passes & 1];
    return SVO_OK;
}

// The list front end for other passes (svo_edit.hip): the argument checks of the list entry points, then keys, sort and
// the leaf pass.  The events are the builder's own, so the times of a build still in flight are taken first.
int svo_build_check_list(svo_ctx *ctx, const uint32_t *depth, const uint32_t *xyz, size_t n) {
    return check_list(ctx, depth, nullptr, false, xyz, n);
}

int svo_build_list_leaves(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, uint32_t depth,
                          uint32_t default_colour, svo_build_leaves *out) {
    int rc = ctx->build ? ctx->build->timer.begin(ctx) : SVO_OK;
    if (rc) return rc;
    rc = list_leaves(ctx, xyz, colours, n, depth, default_colour, 0, true);
    if (rc) return rc;
    svo_build_state *s = ctx->build.get();
    const uint32_t a = ((3 * depth + 7) / 8) & 1;  // the sort's result was in keys[a] / vals[a]: free again, like keys[a ^ 1]
    out->keys = s->keys[2];
    out->colours = s->leaf_colours;
    out->index = s->vals[a ^ 1];
    out->count = s->counts.dev + depth;
    out->range_err = s->counts.dev + kErrSlot;
    out->spare32 = s->vals[a];
    out->spare64[0] = s->keys[0];
    out->spare64[1] = s->keys[1];
    out->items = s->items();
    out->ev_start = s->timer.ev[kEvStart];
    out->ev_keys = s->timer.ev[kEvKeys];
    out->ev_sort = s->timer.ev[kEvSort];
    return SVO_OK;
}

namespace {

constexpr uint64_t kDefaultMaxNodes = 256000000ull;  // procedural.rs:4

// The chunk trees of n voxels: the list front end of svo_nodes_build, the counting passes with the chunk
// runs of every level, one read-back of the counts and runs, the caps, then (the world's directory made when `world` is
// given) the emit into one buffer, the mips and, chunk by chunk in id order, one copy into the pinned stage that
// take(id index, bytes, nodes) consumes.  Nothing is created before every cap has been checked.
template <class Take>
int chunk_build(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_chunk_build_params *p,
                svo_world_writer *world, Take take) {
    const double t0 = svo_now_ms();
    const uint32_t depth = p->depth, wd = p->world_depth, cd = depth - wd, n_chunks = 1u << (3 * wd), row = n_chunks + 1;
    const uint64_t cap = std::min<uint64_t>(p->max_nodes ? p->max_nodes : kDefaultMaxNodes, 1ull << 31);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if (!n) {  // nothing to build: the empty world is its root alone
        if (world && (rc = world->create())) return rc;
        if (ctx->build) memset(ctx->build->cms, 0, sizeof ctx->build->cms);
        return SVO_OK;
    }
    const size_t runs_items = size_t(depth + 1) * row;
    if ((rc = list_leaves(ctx, xyz, colours, n, depth, p->default_colour, runs_items))) return rc;
    svo_build_state *s = ctx->build.get();
    memset(s->cms, 0, sizeof s->cms);
    uint64_t bound[23] = {};
    level_bounds(bound, depth, n);
    ChunkPlan plan{wd, n_chunks, nullptr, 0};
    if ((rc = parent_passes(ctx, depth, std::max(wd, 1u), bound, nullptr, nullptr, 0, &plan))) return rc;
    if ((rc = read_counts(ctx, depth, runs_items))) return rc;
    const uint32_t *m = s->counts.host();

    // every chunk's local level bases (breadth-first: level 1 at 0, level L + 1 behind level L's groups) and its place
    const uint32_t stride = cd + 2;
    std::vector<uint32_t> cbase(size_t(n_chunks) * stride, 0u);
    std::vector<uint64_t> coff(n_chunks, 0ull);
    uint64_t total = 0, largest = 0;
    for (uint32_t c = 0; c < n_chunks; c++) {
        auto count = [&](uint32_t l) -> uint64_t {  // chunk c's nodes at level l
            const uint32_t *r = s->runs_host + size_t(l) * row;
            return l == 0 ? 1u : r[c + 1] - r[c];
        };
        uint32_t *b = cbase.data() + size_t(c) * stride;
        uint64_t at = 0;
        for (uint32_t L = 1; L <= cd; L++) {
            b[L] = (uint32_t)at;
            at += 8 * count(wd + L - 1);
            if (at > cap) {
                uint32_t cx, cy, cz;
                morton_decode(c, wd, cx, cy, cz);
                return svo_fail(ctx, SVO_ERR_CAP, "chunk (" + std::to_string(cx) + ", " + std::to_string(cy) + ", " + std::to_string(cz) +
                                                      ") needs more than " + std::to_string(cap) + " nodes (max_nodes " +
                                                      std::to_string(p->max_nodes) + ", 0 = 256 000 000; at most 2^31)");
            }
        }
        b[cd + 1] = (uint32_t)at;
        coff[c] = total;
        total += at;
        largest = std::max(largest, at);
    }
    if ((rc = svo_grow(ctx, cbase.size(), &s->cbase))) return rc;
    if ((rc = svo_grow(ctx, coff.size(), &s->coff))) return rc;
    if ((rc = svo_grow(ctx, total, &s->nodes))) return rc;
    if ((rc = svo_grow_pinned(ctx, largest * 8, &s->stage))) return rc;
    if (world && (rc = world->create())) return rc;

    // emit and mips
    HIP_TRY(ctx, hipMemcpyAsync(s->cbase, cbase.data(), cbase.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(s->coff, coff.data(), coff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvChunkEmit));
    build_fill_kernel<<<std::max(std::min(svo_div_up(total, kThreads), 65536u), 1u), kThreads, 0, ctx->stream>>>(s->nodes, total);
    HIP_TRY(ctx, hipGetLastError());
    for (uint32_t l = 1; l <= depth; l++) bound[l] = m[l];
    plan.nodes = s->nodes;
    plan.n_nodes = total;
    if ((rc = parent_passes(ctx, depth, wd + 1, bound, nullptr, nullptr, 0, &plan))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvChunkEmitEnd));
    for (uint32_t l = depth - 1; l > wd; l--) {  // bottom-up; level `depth` is all leaves
        const uint32_t lanes = 8u * m[l - 1];
        build_mip_kernel<<<svo_div_up(lanes, kThreads), kThreads, 0, ctx->stream>>>(s->nodes, s->coff, s->cbase, s->runs + size_t(l - 1) * row,
                                                                                     n_chunks, stride, l - wd, lanes);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvChunkMips));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    // chunks in id order: (cx * side + cy) * side + cz, chunk index = Morton code of (cx, cy, cz)
    const uint32_t side = 1u << wd;
    double copy_ms = 0, take_ms = 0;
    for (uint32_t id = 0; id < n_chunks; id++) {
        const uint32_t c = (uint32_t)morton_encode(id / (side * side), id / side % side, id % side, wd);
        const uint64_t nodes = cbase[size_t(c) * stride + cd + 1];
        if (!nodes) continue;
        double t = svo_now_ms();
        HIP_TRY(ctx, hipMemcpyAsync(s->stage, s->nodes + coff[c], nodes * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        copy_ms += svo_now_ms() - t;
        t = svo_now_ms();
        if ((rc = take(id, (const uint8_t *)s->stage.get(), nodes))) return rc;
        take_ms += svo_now_ms() - t;
    }
    for (int k = 0; k < 6; k++) HIP_TRY(ctx, hipEventElapsedTime(&s->cms[k], s->timer.ev[kChunkSlots[k].first], s->timer.ev[kChunkSlots[k].last]));
    s->cms[6] = float(copy_ms);
    s->cms[7] = float(take_ms);
    s->cms[8] = float(svo_now_ms() - t0);
    return SVO_OK;
}

// top_mip of a chunk: the mip of its root group (nodes 0..7 in the <id>.bin layout)
void chunk_top_mip(const uint8_t *bytes, uint8_t rgb[3]) {
    uint32_t v[8];
    for (int c = 0; c < 8; c++) v[c] = bytes[8 * c + 4] | bytes[8 * c + 5] << 8 | bytes[8 * c + 6] << 16;
    const uint32_t t = mip_of(v);
    rgb[0] = t & 0xFFu;
    rgb[1] = t >> 8 & 0xFFu;
    rgb[2] = t >> 16 & 0xFFu;
}

}  // namespace

// ---- the world writer (svo_ctx.h): the layout of a generated world's directory, for svo_world_build below and
// svo_world_generate (svo_proc.hip) ----
svo_world_writer::svo_world_writer(svo_ctx *ctx, svo_world *w, uint32_t world_depth)
    : ctx(ctx), w(w), world_depth(world_depth), path(svo_world_path(w)) {}

svo_world_writer::~svo_world_writer() { svo_cpu_octree_free(root); }

int svo_world_writer::refuse_existing() {
    if (path.empty()) return svo_fail(ctx, SVO_ERR_ARG, "world has no path");
    struct stat st;
    if (stat(path.c_str(), &st) == 0) return svo_fail(ctx, SVO_ERR_ARG, "File already exists");  // World::generate_world's words
    return SVO_OK;
}

int svo_world_writer::create() {
    int rc = refuse_existing();
    if (rc) return rc;
    if (mkdir(path.c_str(), 0777) != 0) return svo_fail(ctx, SVO_ERR_STATE, "cannot create " + path + ": " + strerror(errno));
    root = svo_cpu_octree_new(0);
    return SVO_OK;
}

int svo_world_writer::add_chunk(uint32_t i, const void *bytes, uint64_t n_nodes) {
    const uint32_t id = SVO_CHUNK_OFFSET / 2 + i, side = 1u << world_depth;
    uint8_t top[3];
    chunk_top_mip((const uint8_t *)bytes, top);
    if (svo_world_write_chunk(w, id, bytes, n_nodes * 8, top) != 0)
        return svo_fail(ctx, SVO_ERR_STATE, std::string("save: ") + svo_world_last_error(w));
    const float voxel = 2.0f / float(side);
    const float pos[3] = {float(i / (side * side)) * voxel - 1.0f, float(i / side % side) * voxel - 1.0f, float(i % side) * voxel - 1.0f};
    svo_cpu_octree_put_in_block(root, pos, id, world_depth);
    return SVO_OK;
}

int svo_world_writer::finish(float *mip_ms, float *save_ms) {
    svo_world_insert(w, 0, root);  // (the world owns it from here)
    root = nullptr;
    double t = svo_now_ms();
    if (svo_world_generate_mip_tree(w, 0, nullptr) != 0) return svo_fail(ctx, SVO_ERR_STATE, std::string("mips: ") + svo_world_last_error(w));
    *mip_ms = float(svo_now_ms() - t);
    t = svo_now_ms();
    if (svo_world_save_chunk(w, 0) != 0) return svo_fail(ctx, SVO_ERR_STATE, std::string("save: ") + svo_world_last_error(w));
    *save_ms = float(svo_now_ms() - t);
    return SVO_OK;
}

extern "C" {

int svo_nodes_build(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_build_params *p,
                    uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    int rc = check_list(ctx, p ? &p->depth : nullptr, nullptr, false, xyz, n);
    if (rc) return rc;
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if ((rc = svo_check_store(ctx))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!n) return build_empty(ctx, p, n_words_out);
    const double t0 = svo_now_ms();
    if ((rc = list_leaves(ctx, xyz, colours, n, p->depth, p->default_colour, 0))) return rc;
    return finish(ctx, p, n, t0, true, n_words_out);
}

int svo_nodes_build_dense(svo_ctx *ctx, const uint32_t *grid, const svo_build_params *p, uint64_t *n_words_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_words_out) *n_words_out = 0;
    int rc = check_depth(ctx, p ? &p->depth : nullptr, 10);
    if (rc) return rc;
    if (!grid) return svo_fail(ctx, SVO_ERR_ARG, "null grid");
    if (!n_words_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_words_out");
    if ((rc = svo_check_store(ctx))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t depth = p->depth;
    const uint64_t cells = 1ull << (3 * depth);
    // every leaf takes a word: a grid with more solid cells than the limit has words fails the cap, so the leaf level
    // needs no more room than that
    const uint64_t room = std::max<uint64_t>(std::min(cells, word_limit(ctx, p)), 1);
    if ((rc = ensure_state(ctx, room, cells, 0))) return rc;
    svo_build_state *s = ctx->build.get();
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    HIP_TRY(ctx, s->counts.zero(ctx));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvKeys));
    HIP_TRY(ctx, s->timer.mark(ctx, kEvSort));
    LevelIn in{};
    in.colours = grid;
    in.m_max = (uint32_t)cells;
    in.depth = depth;
    LevelOut out{};
    out.keys = s->keys[2];
    out.colours = s->leaf_colours;
    out.cap = (uint32_t)s->items();
    if ((rc = level_pass<kDense>(ctx, in, out, cells, s->counts.dev + depth))) return rc;
    return finish(ctx, p, cells, t0, false, n_words_out);
}

int svo_build_timing(svo_ctx *ctx, float ms_out[SVO_BUILD_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->build) return svo_fail(ctx, SVO_ERR_STATE, "no tree built on this context yet");
    return ctx->build->timer.read(ctx, ms_out);
}

int svo_cpu_octree_build(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_chunk_build_params *p,
                         svo_cpu_octree **out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!out) return svo_fail(ctx, SVO_ERR_ARG, "null output");
    *out = nullptr;
    int rc = check_list(ctx, p ? &p->depth : nullptr, p, false, xyz, n);
    if (rc) return rc;
    svo_cpu_octree *tree = nullptr;
    rc = chunk_build(ctx, xyz, colours, n, p, nullptr, [&](uint32_t, const uint8_t *bytes, uint64_t nodes) -> int {
        char why[128] = "";
        tree = svo_cpu_octree_from_bin(bytes, nodes * 8, why, sizeof why);
        if (!tree) return svo_fail(ctx, SVO_ERR_STATE, std::string("emitted tree rejected: ") + why);
        uint8_t top[3];
        chunk_top_mip(bytes, top);
        svo_cpu_octree_set_top_mip(tree, top);
        return SVO_OK;
    });
    if (rc) {
        svo_cpu_octree_free(tree);
        return rc;
    }
    *out = tree;
    return SVO_OK;
}

int svo_world_build(svo_ctx *ctx, svo_world *w, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_chunk_build_params *p) {
    if (!ctx) return SVO_ERR_ARG;
    if (!w) return svo_fail(ctx, SVO_ERR_ARG, "null world");
    int rc = check_list(ctx, p ? &p->depth : nullptr, p, true, xyz, n);
    if (rc) return rc;
    svo_world_writer world(ctx, w, p->world_depth);
    if ((rc = world.refuse_existing())) return rc;
    rc = chunk_build(ctx, xyz, colours, n, p, &world,
                     [&](uint32_t i, const uint8_t *bytes, uint64_t nodes) -> int { return world.add_chunk(i, bytes, nodes); });
    if (rc) return rc;
    float mip_ms = 0.0f, save_ms = 0.0f;
    if ((rc = world.finish(&mip_ms, &save_ms))) return rc;
    if (ctx->build) {
        ctx->build->cms[7] += mip_ms + save_ms;
        ctx->build->cms[8] += mip_ms + save_ms;
    }
    return SVO_OK;
}

int svo_world_build_timing(svo_ctx *ctx, float ms_out[SVO_WORLD_BUILD_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->build) return svo_fail(ctx, SVO_ERR_STATE, "no chunk tree built on this context yet");
    memcpy(ms_out, ctx->build->cms, sizeof ctx->build->cms);
    return SVO_OK;
}

}  // extern "C"

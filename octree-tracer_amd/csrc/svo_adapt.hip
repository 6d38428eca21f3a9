// svo_adapt.hip -- the adaptive subdivide / unsubdivide step on the GPU: the device form of
// svo_adaptive_subdivide(sorted(sub)) followed by svo_adaptive_unsubdivide(sorted(unsub)), bit for bit, on state that
// stays in device memory: the node buffer, node positions, the hole stack, the tree length and a mirror of the world's
// resident chunks.  The host loop is sequential; here every list entry is one lane, and what the sequential order
// decides is recovered with scans and rank look-ups in the sorted list:
//
//   subdivide    plan (read only): per entry the octree walk to its voxel depth, the world walk, the source group of
//                the 8 children -- or a chunk the host must load first (the lowest-ranked entry that references a
//                missing chunk loads it and is skipped; the host loads, the mirror grows, the plan runs again).  Entries
//                that would make the passes depend on each other are refused before anything is written.  Then an
//                exclusive scan of the success flags gives the k-th success hole_stack[H-1-k] or a fresh group at
//                len + 8 (k - H), and the apply writes the words and positions.
//   unsubdivide  plan (read only, on the words the subdivide pass left): the octree walk stops at the first node that is
//                a leaf or a successful entry of rank <= its own (nested collapses in one pass), the world walk gives the
//                written colour and the chunk to drop; a scan gives the hole pushes in list order; the apply writes.
//
// Both lists are sorted first with the tree builder's radix sort (svo_build.hip).
//
// svo_adaptive_expand is the device form of svo_world_expand on the same state: the host's frontier walk
// taken level by level.  A kernel lists the tree's leaves with their depths in index order; per level a kernel keeps
// the leaves the view refines (already sorted, so no radix sort), the subdivide pass above runs on them with a success
// limit for the word cap, and a kernel writes the next frontier: the 8 slots of every group the pass made, in order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "svo_ctx.h"
#include "svo_rules.h"  // (the walks, pointer classes and view rule the host path runs too)
#include "svo_scan.h"   // (kThreads; tiles of kTile items for the expand's compactions)

namespace {

using svo_rules::leaf_word;
using svo_rules::pos_offset;
using svo_rules::Vec3;

constexpr uint32_t kVoxelOff = SVO_VOXEL_OFFSET;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kFailed = 0xFFFFFFFEu;  // Chunk::rank of a chunk whose load failed in this pass (not resident)
constexpr uint32_t kMaxTreeDepth = 31;     // pos_offset's 1 << depth
constexpr uint32_t kMaxRank = 1u << 24;    // ranks are packed with an 8-bit code into one word
constexpr uint32_t kListCap = 1024000;     // the scan lists (adaptive.rs:3-4)

// per-entry outcome codes; errors are packed as rank << 8 | code so that an atomicMin keeps the first in list order
enum Code : uint32_t {
    kSkip = 0,
    kDone = 1,
    kErrRange = 2,    // entry >= len (refusal / error)
    kErrDup = 3,      // duplicated subdivide entry (refusal)
    kErrDep = 4,      // an entry's walk ends at another listed entry (refusal)
    kErrOrder = 5,    // a chunk loaded in this pass by a later entry (refusal)
    kErrWalk = 6,     // the octree walk left the array or went deeper than 31 levels
    kErrWorld = 7,    // world walk left the loaded chunks
    kErrPast = 8,     // child pointer past the chunk
    kErrNoPos = 9,    // unsubdivide of a node without position
};

// the host shadow of one resident chunk; the device table is sorted by id
struct Chunk {
    uint32_t id, first, count, rank;  // rank: kNone = resident before this pass, kFailed, else the entry that loaded it
};

struct Status {
    uint32_t refuse, err;  // rank << 8 | code, kNone when clear
    uint32_t n_req;        // chunk requests (subdivide plan)
    uint32_t removals;     // unsubdivide plan: some entry drops a resident chunk
    uint32_t popped_hit;   // subdivide: an entry lies in a group popped in this pass
    uint32_t total;        // the scan's total (successes)
    uint32_t pad[2];
};

__device__ inline bool is_leaf(uint32_t w) { return svo_rules::word_is_leaf(w); }

__device__ inline uint32_t lower_bound(const uint32_t *a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline uint32_t find_chunk(const Chunk *tab, uint32_t n, uint32_t id) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].id < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && tab[lo].id == id ? lo : kNone;
}

__device__ inline void report(uint32_t *slot, uint32_t rank, uint32_t code) { atomicMin(slot, rank << 8 | code); }

// Octree::find_voxel from the root (svo_rules::descend), until stop(index, word): the stopping depth (0: the walk left
// [0, len) or went deeper than 31 levels) and index.
template <class Stop>
__device__ inline uint32_t tree_walk(const uint32_t *nodes, uint32_t len, Vec3 p, Stop stop, uint32_t &at) {
    uint32_t base = 0;
    Vec3 c;
    for (uint32_t depth = 1; depth <= kMaxTreeDepth; depth++) {
        at = base + svo_rules::descend(p, c, depth);
        if (at >= len) return 0;
        const uint32_t w = nodes[at];
        if (stop(at, w)) return depth;
        base = w >> 4;
    }
    return 0;
}

// The mirror as svo_rules::world_walk sees it: a chunk's handle is its table slot and the entry there, loaded once when
// the walk enters the chunk; is_resident(slot) says whether an entered chunk counts as loaded.
template <class Resident>
struct MirrorChunks {
    struct In {
        uint32_t slot;
        Chunk c;
    };
    const Chunk *tab;
    uint32_t n_tab;
    const uint2 *wn;
    Resident is_resident;
    __device__ In find(uint32_t id) const {
        const uint32_t slot = find_chunk(tab, n_tab, id);
        return {slot, slot != kNone ? tab[slot] : Chunk{}};
    }
    __device__ bool resident(const In &in) const { return in.slot != kNone && is_resident(in.slot); }
    __device__ uint32_t count(const In &in) const { return in.c.count; }
    __device__ uint32_t pointer(const In &in, uint32_t i) const { return wn[in.c.first + i].x; }
};

// World::find_voxel over the mirror, to max_depth: the mirror index of the node it ends on (and its chunk's table slot),
// or kNone when it leaves the loaded chunks (kErrWorld).
template <class Resident>
__device__ inline uint32_t world_walk(const Chunk *tab, uint32_t n_tab, const uint2 *wn, Vec3 p, uint32_t max_depth,
                                      Resident resident, uint32_t &slot) {
    const auto at = svo_rules::world_walk(MirrorChunks<Resident>{tab, n_tab, wn, resident}, p, max_depth);
    slot = at.in.slot;
    return at.ok ? at.in.c.first + at.index : kNone;
}

struct Tree {
    uint32_t *nodes;
    float *pos;  // 3 per node
    uint32_t len;
};

__device__ inline Vec3 load_pos(const float *pos, uint32_t i) {
    return {pos[3 * size_t(i)], pos[3 * size_t(i) + 1], pos[3 * size_t(i) + 2]};
}

// ---- subdivide ----
// res[k] = code | voxel_depth << 8; src[k] = mirror index of the children's 8 world nodes; flag[k] = success.
__global__ __launch_bounds__(kThreads) void sub_plan_kernel(Tree t, const uint32_t *list, uint32_t n, const Chunk *tab,
                                                            uint32_t n_tab, const uint2 *wn, uint32_t *res, uint32_t *src,
                                                            uint32_t *flag, uint32_t *req, Status *st) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    res[k] = kSkip;
    flag[k] = 0;
    const uint32_t node = list[k];
    if (node >= t.len) return report(&st->refuse, k, kErrRange);
    if (k > 0 && list[k - 1] == node) return report(&st->refuse, k, kErrDup);
    if (!is_leaf(t.nodes[node])) return;  // "Doubleup!" (adaptive.rs:32-35)
    const Vec3 p = load_pos(t.pos, node);
    uint32_t at = 0;
    const uint32_t vd = tree_walk(t.nodes, t.len, p, [](uint32_t, uint32_t w) { return is_leaf(w); }, at);
    if (!vd) return report(&st->err, k, kErrWalk);
    if (at != node) {  // the walk ends on another leaf: if that one is listed, the host's order matters
        const uint32_t j = lower_bound(list, n, at);
        if (j < n && list[j] == at) return report(&st->refuse, k, kErrDep);
    }
    // a chunk loaded in this pass is resident for the entries after the one that loaded it
    auto resident = [&](uint32_t s) { const uint32_t r = tab[s].rank; return r == kNone || (r != kFailed && r < k); };
    uint32_t slot;
    const uint32_t wi = world_walk(tab, n_tab, wn, p, vd, resident, slot);
    if (wi == kNone) return report(&st->err, k, kErrWorld);
    const uint32_t ptr = wn[wi].x;
    uint32_t first;
    if (svo_rules::ptr_is_group(ptr)) {  // adaptive.rs:42-48
        if (ptr + 8u > tab[slot].count) return report(&st->err, k, kErrPast);
        first = tab[slot].first + ptr;
    } else if (svo_rules::ptr_is_chunk(ptr)) {  // :49-58
        const uint32_t id = svo_rules::ptr_chunk_id(ptr), s = find_chunk(tab, n_tab, id);
        if (s == kNone) {  // not loaded: the lowest-ranked such entry loads it (the host takes the minimum) and is skipped
            const uint32_t q = atomicAdd(&st->n_req, 1u);
            req[2 * q] = id;
            req[2 * q + 1] = k;
            return;
        }
        const Chunk c = tab[s];
        if (c.rank == kFailed || c.rank == k) return;  // a failed load / the entry that loaded it
        if (c.rank != kNone && c.rank > k) return report(&st->refuse, k, kErrOrder);
        if (c.count < 8) return;  // nodes dropped to save memory (world.rs:134)
        first = c.first;
    } else {
        return;
    }
    res[k] = kDone | vd << 8;
    src[k] = first;
    flag[k] = 1;
}

// An entry inside a group this pass pops would be written by another entry: refuse.  (Fresh groups lie past len.)
__global__ __launch_bounds__(kThreads) void sub_popped_kernel(const uint32_t *holes, uint32_t n_holes, const uint32_t *list,
                                                              uint32_t n, const uint32_t *total, Status *st) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t pops = min(*total, n_holes);
    if (j >= pops) return;
    const uint32_t g = holes[n_holes - 1 - j];
    const uint32_t i = lower_bound(list, n, g);
    if (i < n && list[i] < g + 8u) st->popped_hit = 1;
}

__global__ __launch_bounds__(kThreads) void sub_apply_kernel(Tree t, const uint32_t *list, uint32_t n, const uint32_t *res,
                                                             const uint32_t *src, const uint32_t *rank, const uint32_t *holes,
                                                             uint32_t n_holes, const uint2 *wn, uint32_t capacity, uint32_t limit,
                                                             Status *st) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || (res[k] & 0xFFu) != kDone) return;
    const uint32_t s = rank[k];
    if (s >= limit) return;  // (svo_adaptive_expand: behind the word cap)
    const uint32_t g = s < n_holes ? holes[n_holes - 1 - s] : t.len + 8u * (s - n_holes);
    if (g >= capacity || capacity - g < 8u) return report(&st->err, k, kErrRange);
    const uint32_t node = list[k], depth = (res[k] >> 8) + 1u, first = src[k];
    const Vec3 p = load_pos(t.pos, node);
    t.nodes[node] = g << 4;
    for (uint32_t i = 0; i < 8; i++) {
        const Vec3 o = pos_offset(i, depth);
        t.nodes[g + i] = leaf_word(wn[first + i].y);
        float *q = t.pos + 3 * size_t(g + i);
        q[0] = p.x + o.x;
        q[1] = p.y + o.y;
        q[2] = p.z + o.z;
    }
}

// ---- unsubdivide ----
__global__ __launch_bounds__(kThreads) void unsub_mark_kernel(const uint32_t *list, uint32_t n, uint32_t len, uint32_t *bits) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n && list[k] < len) atomicOr(&bits[list[k] >> 5], 1u << (list[k] & 31u));
}

// res[k] = code | voxel_depth << 8 (kDone: collapses an interior node, pushes its group); val[k] = the word written;
// grp[k] = the group pushed; flag[k] = success.  rm[slot] = lowest rank that drops the chunk.
__global__ __launch_bounds__(kThreads) void unsub_plan_kernel(Tree t, const uint32_t *list, uint32_t n, const uint32_t *bits,
                                                              const Chunk *tab, uint32_t n_tab, const uint2 *wn, uint32_t *res,
                                                              uint32_t *val, uint32_t *grp, uint32_t *flag, uint32_t *rm,
                                                              Status *st) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    res[k] = kSkip;
    flag[k] = 0;
    const uint32_t node = list[k];
    if (node >= t.len) return report(&st->err, k, kErrRange);
    const uint32_t w = t.nodes[node];
    const bool first_of_run = k == 0 || list[k - 1] != node;  // a repeat sees the leaf its first occurrence left
    const bool collapse = !is_leaf(w) && first_of_run;
    const Vec3 p = load_pos(t.pos, node);
    if (collapse && p.x == 0.0f && p.y == 0.0f && p.z == 0.0f) return report(&st->err, k, kErrNoPos);
    // the host walks the tree after entries 0..k: a node on the path is a leaf if it was one after the subdivide pass or
    // is an interior entry of rank <= k (collapsed by then)
    auto stop = [&](uint32_t at, uint32_t wa) {
        if (is_leaf(wa)) return true;
        if (!((bits[at >> 5] >> (at & 31u)) & 1u)) return false;
        return lower_bound(list, n, at) <= k;
    };
    uint32_t at = 0;
    const uint32_t vd = tree_walk(t.nodes, t.len, p, stop, at);
    if (!vd) return report(&st->err, k, kErrWalk);
    uint32_t slot;
    const uint32_t wi = world_walk(tab, n_tab, wn, p, vd, [](uint32_t) { return true; }, slot);
    if (wi == kNone) return report(&st->err, k, kErrWorld);
    const uint2 wnode = wn[wi];
    if (svo_rules::ptr_is_chunk(wnode.x) && svo_rules::chunk_is_streamed(svo_rules::ptr_chunk_id(wnode.x))) {  // adaptive.rs:104-110
        const uint32_t s = find_chunk(tab, n_tab, svo_rules::ptr_chunk_id(wnode.x));
        if (s != kNone) {
            atomicMin(&rm[s], k);
            st->removals = 1;
        }
    }
    res[k] = (collapse ? kDone : kSkip) | vd << 8;
    val[k] = leaf_word(wnode.y);
    grp[k] = w >> 4;
    flag[k] = collapse ? 1u : 0u;
}

// A world walk that enters a chunk an earlier entry dropped fails, as on the host.  Run only when something was dropped.
__global__ __launch_bounds__(kThreads) void unsub_check_kernel(Tree t, const uint32_t *list, uint32_t n, const uint32_t *res,
                                                               const Chunk *tab, uint32_t n_tab, const uint2 *wn,
                                                               const uint32_t *rm, Status *st) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const Vec3 p = load_pos(t.pos, list[k]);
    uint32_t slot;
    const uint32_t wi = world_walk(tab, n_tab, wn, p, res[k] >> 8, [&](uint32_t s) { return rm[s] >= k; }, slot);
    if (wi == kNone) report(&st->err, k, kErrWorld);
}

__global__ __launch_bounds__(kThreads) void unsub_apply_kernel(Tree t, const uint32_t *list, uint32_t n, const uint32_t *res,
                                                               const uint32_t *val, const uint32_t *grp, const uint32_t *rank,
                                                               uint32_t *holes, uint32_t n_holes, uint32_t hole_cap) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || (k > 0 && list[k - 1] == list[k])) return;
    t.nodes[list[k]] = val[k];
    if ((res[k] & 0xFFu) == kDone && n_holes + rank[k] < hole_cap) holes[n_holes + rank[k]] = grp[k];
}

// ---- expand ----
// A frontier entry is node index | depth << 27: an index is below 2^27 (SVO_VOXEL_OFFSET), a depth at most 31.
constexpr uint32_t kDepthShift = 27, kIndexMask = (1u << kDepthShift) - 1u;

// A stable compaction of the words in[0, n) as a tile pass (svo_scan.h), its items and its emit in one: the state is a
// thread's words and the mask of those that keep(word) keeps, and emit(i, word, rank) is called for every kept word, which
// is in registers from the test on.
struct KeptWords {
    uint32_t w[kPer], kept;
};

template <class Keep, class Emit>
struct Compaction {
    const uint32_t *in;
    Keep keep;
    Emit emit;
    __device__ KeptWords load(uint32_t i0, uint32_t n) const {
        KeptWords s{};
        for (uint32_t j = 0; j < kPer; j++) {
            s.w[j] = i0 + j < n ? in[i0 + j] : 0u;
            if (i0 + j < n && keep(s.w[j])) s.kept |= 1u << j;
        }
        return s;
    }
    __device__ uint32_t count(const KeptWords &s) const { return __popc(s.kept); }
    __device__ void operator()(const Compaction &, uint32_t i0, const KeptWords &s, uint32_t r) const {
        for (uint32_t j = 0; j < kPer; j++)
            if ((s.kept >> j) & 1u) emit(i0 + j, s.w[j], r++);
    }
};

// The initial frontier: every leaf of [0, len) with the depth of the walk to its position, in index order.  The count
// only tests the words, the emit walks.
struct LeafWord {
    __device__ bool operator()(uint32_t w) const { return is_leaf(w); }
};

struct EmitLeaf {
    Tree t;
    uint32_t *out, out_cap;
    Status *st;
    __device__ void operator()(uint32_t i, uint32_t, uint32_t r) const {
        uint32_t at = 0;
        const uint32_t d = tree_walk(t.nodes, t.len, load_pos(t.pos, i), [](uint32_t, uint32_t w) { return is_leaf(w); }, at);
        if (!d) report(&st->err, min(i, kMaxRank - 1u), kErrWalk);
        if (r < out_cap) out[r] = i | d << kDepthShift;  // (always: the counts come from the same words)
    }
};

// svo_world_expand's rule for one frontier leaf: deeper than max_depth never; with a camera, only while
// svo_rules::lod_refines says so for the leaf's cube, centre +- half edge.
struct View {
    float cam[3], lod_c;
    uint32_t max_depth, use_cam;
};

struct ViewRefines {
    const float *pos;
    View v;
    __device__ bool operator()(uint32_t entry) const {
        const uint32_t d = entry >> kDepthShift;
        if (d >= v.max_depth) return false;
        if (!v.use_cam) return true;
        const Vec3 c = load_pos(pos, entry & kIndexMask);
        const float h = 1.0f / float(1u << d);  // half edge of a depth-d cube
        const float lo[3] = {c.x - h, c.y - h, c.z - h}, hi[3] = {c.x + h, c.y + h, c.z + h};
        return svo_rules::lod_refines(v.cam, lo, hi, d, v.lod_c);
    }
};

// the passing node indices, in frontier order, into list[0, total) (rank < n: at most one index per frontier entry)
struct EmitCandidate {
    uint32_t *list;
    __device__ void operator()(uint32_t, uint32_t entry, uint32_t r) const { list[r] = entry & kIndexMask; }
};

// Success s (< limit) of the pass made the group at len_before + 8 s out of a leaf of depth d: its 8 slots, depth d + 1,
// are entries [8 s, 8 s + 8) of the next frontier.  rank is the pass's scanned flag array.
__global__ __launch_bounds__(kThreads) void next_frontier_kernel(uint32_t n, const uint32_t *res, const uint32_t *rank,
                                                                 uint32_t limit, uint32_t len_before, uint32_t *out) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n || (res[k] & 0xFFu) != kDone) return;
    const uint32_t s = rank[k];
    if (s >= limit) return;
    const uint32_t g = len_before + 8u * s, d = (res[k] >> 8) + 1u;
    for (uint32_t i = 0; i < 8; i++) out[8u * s + i] = (g + i) | d << kDepthShift;
}

}  // namespace

struct svo_adapt_state {
    svo_world *world = nullptr;
    uint32_t *nodes_at_attach = nullptr;  // the node buffer the state belongs to
    size_t capacity = 0;                  // the node buffer's at attach
    svo_dev<float> pos;                   // 3 per node
    svo_dev<uint32_t> holes;
    uint32_t n_holes = 0;
    uint32_t len = 0;
    // world mirror: nodes {pointer, rgb} of every resident chunk, concatenated; table sorted by id
    svo_dev<uint2> wn;
    size_t wn_used = 0;  // nodes of the mirror in use
    std::vector<Chunk> tab;
    svo_dev<Chunk> tab_dev;
    svo_dev<uint32_t> rm;  // per table slot: lowest unsubdivide rank that drops it
    // per-entry workspace
    svo_dev<uint32_t> list[2];  // sorted subdivide / unsubdivide lists
    svo_dev<uint32_t> res, src, val, flag;
    svo_dev<uint32_t> req;  // 2 per entry (grow_entries)
    svo_dev<uint32_t> bits;
    svo_mirrored<Status> st;                // one Status
    svo_pinned<uint32_t> counts_host;     // scan list counts
    std::vector<uint32_t> removed;
    svo_events<4> ev;  // start, sorted, subdivided, unsubdivided
    float ms[SVO_ADAPT_TIMES] = {};
    // svo_adaptive_expand: this level's frontier and the next one's, the compactions' tile sums
    svo_dev<uint32_t> frontier[2];
    svo_dev<uint32_t> tiles;
    float expand_ms[SVO_ADAPT_EXPAND_TIMES] = {};

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, ev.create());
        if (int rc = st.alloc(ctx, 1)) return rc;
        HIP_TRY(ctx, counts_host.alloc(2));
        return SVO_OK;
    }
};

namespace {

// the table is sorted by id, and an id is in it once
bool by_id(const Chunk &x, const Chunk &y) { return x.id < y.id; }
void table_insert(std::vector<Chunk> &tab, const Chunk &c) { tab.insert(std::upper_bound(tab.begin(), tab.end(), c, by_id), c); }

// the table (and the rank array sized to it) to the device; blocking, so the host vector may change afterwards
int upload_table(svo_ctx *ctx) {
    svo_adapt_state *a = ctx->adapt.get();
    int rc = svo_grow(ctx, std::max<size_t>(a->tab.size(), 16), &a->tab_dev);
    if (rc) return rc;
    if ((rc = svo_grow(ctx, std::max<size_t>(a->tab.size(), 16), &a->rm))) return rc;
    if (!a->tab.empty())
        HIP_TRY(ctx, hipMemcpyAsync(a->tab_dev, a->tab.data(), a->tab.size() * sizeof(Chunk), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

int put_chunk_nodes(svo_ctx *ctx, const svo_cpu_octree *t, uint32_t at, size_t count) {
    if (!count) return SVO_OK;
    std::vector<uint32_t> ptr(count);
    std::vector<uint8_t> rgb(3 * count);
    svo_cpu_octree_raw(t, ptr.data(), rgb.data());
    std::vector<uint2> nodes(count);
    for (size_t i = 0; i < count; i++)
        nodes[i] = make_uint2(ptr[i], uint32_t(rgb[3 * i]) << 16 | uint32_t(rgb[3 * i + 1]) << 8 | rgb[3 * i + 2]);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->adapt->wn + at, nodes.data(), count * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

// The whole mirror from the host world (attach, or a load that does not fit): every chunk, compact, twice the room.
int rebuild_mirror(svo_ctx *ctx, size_t extra) {
    svo_adapt_state *a = ctx->adapt.get();
    std::vector<uint32_t> ids(svo_world_chunk_ids(a->world, nullptr, 0));
    svo_world_chunk_ids(a->world, ids.data(), ids.size());
    std::vector<Chunk> old;
    old.swap(a->tab);
    size_t total = 0;
    for (uint32_t id : ids) total += svo_cpu_octree_len(svo_world_chunk(a->world, id));
    if (total + extra >= kNone) return svo_fail(ctx, SVO_ERR_CAP, "the world mirror would pass 2^32 nodes");
    if (a->wn.size() < total + extra) {
        const int rc = svo_grow(ctx, std::min<size_t>(2 * (total + extra) + 4096, kNone - 1), &a->wn);
        if (rc) return rc;
    }
    a->wn_used = 0;
    for (uint32_t id : ids) {
        const svo_cpu_octree *t = svo_world_chunk(a->world, id);
        const size_t cnt = svo_cpu_octree_len(t);
        uint32_t rank = kNone;
        for (const Chunk &c : old)
            if (c.id == id) rank = c.rank;  // (a rebuild inside a subdivide pass keeps the load ranks)
        a->tab.push_back({id, (uint32_t)a->wn_used, (uint32_t)cnt, rank});
        int rc = put_chunk_nodes(ctx, t, (uint32_t)a->wn_used, cnt);
        if (rc) return rc;
        a->wn_used += cnt;
    }
    for (const Chunk &c : old)
        if (c.rank == kFailed) a->tab.push_back(c);
    std::sort(a->tab.begin(), a->tab.end(), by_id);
    return upload_table(ctx);
}

// Chunk `id` was just loaded into the host world by entry `rank`: into the mirror and the table.
int mirror_add(svo_ctx *ctx, uint32_t id, uint32_t rank) {
    svo_adapt_state *a = ctx->adapt.get();
    const svo_cpu_octree *t = svo_world_chunk(a->world, id);
    const size_t cnt = svo_cpu_octree_len(t);
    if (a->wn_used + cnt > a->wn.size()) {
        table_insert(a->tab, {id, 0, 0, rank});  // (the rebuild reads its nodes from the world and keeps the rank)
        return rebuild_mirror(ctx, 0);
    }
    int rc = put_chunk_nodes(ctx, t, (uint32_t)a->wn_used, cnt);
    if (rc) return rc;
    table_insert(a->tab, {id, (uint32_t)a->wn_used, (uint32_t)cnt, rank});
    a->wn_used += cnt;
    return SVO_OK;
}

const char *code_text(uint32_t code) {
    switch (code) {
        case kErrRange: return "node index past the octree";
        case kErrDup: return "a subdivide entry is listed twice";
        case kErrDep: return "a subdivide entry's walk ends at another listed entry";
        case kErrOrder: return "a chunk is first referenced through another chunk loaded in the same pass";
        case kErrWalk: return "the octree walk left the array or passed 31 levels";
        case kErrWorld: return "world walk left the loaded chunks";
        case kErrPast: return "child pointer past the chunk";
        case kErrNoPos: return "Tried to unsubdivide a node without position!";
        default: return "unknown";
    }
}

int entry_fail(svo_ctx *ctx, int code, uint32_t packed, const char *pass) {
    return svo_fail(ctx, code, std::string(pass) + " entry " + std::to_string(packed >> 8) + ": " + code_text(packed & 0xFFu) +
                                   (code == SVO_ERR_STATE ? " (this list needs the sequential host path, svo_adaptive_subdivide)" : ""));
}

int read_status(svo_ctx *ctx, const uint32_t *total_dev) {
    svo_adapt_state *a = ctx->adapt.get();
    if (total_dev) HIP_TRY(ctx, hipMemcpyAsync(&a->st.dev->total, total_dev, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    return a->st.read(ctx);
}

int clear_status(svo_ctx *ctx) {
    Status s{};
    s.refuse = s.err = kNone;
    *ctx->adapt->st.host() = s;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->adapt->st.dev, ctx->adapt->st.host(), sizeof(Status), hipMemcpyHostToDevice, ctx->stream));
    return SVO_OK;
}

Tree tree_of(svo_ctx *ctx) { return Tree{ctx->nodes, ctx->adapt->pos, ctx->adapt->len}; }

// what a buffer of `have` items grows to for `want`: at least twice its size, so a run of growing levels reallocates rarely
size_t grown(size_t have, size_t want) { return have >= want ? have : std::max(want, 2 * have); }
// ... and the hole stack: twice what it needs, so the passes that follow push without growing it again
size_t grown_stack(size_t have, size_t want) { return have >= want ? have : 2 * want; }

// the per-entry workspace for `items` entries, and req's two words for each; flag is allocated last, so its size is
// the room of all of them
int grow_entries(svo_ctx *ctx, size_t items) {
    svo_adapt_state *a = ctx->adapt.get();
    const int rc = svo_grow(ctx, items, &a->list[0], &a->list[1], &a->res, &a->src, &a->val, &a->flag);
    return rc ? rc : svo_grow(ctx, 2 * items, &a->req);
}

// ---- the subdivide pass over the sorted list a->list[0][0, n) ----
// Only the first `limit` successes in list order are applied (svo_adaptive_expand's word cap; kNone: all of them).
int subdivide_pass(svo_ctx *ctx, uint32_t n, uint32_t limit, svo_adaptive_result *out) {
    svo_adapt_state *a = ctx->adapt.get();
    const uint32_t *list = a->list[0], grid = svo_div_up(n, kThreads);
    int rc;
    // plan until no entry asks for a chunk that is not in the table (every load makes a new chunk resident for the
    // entries after its loader, whose walks may then reach further)
    for (int round = 0;; round++) {
        if ((rc = clear_status(ctx))) return rc;
        sub_plan_kernel<<<grid, kThreads, 0, ctx->stream>>>(tree_of(ctx), list, n, a->tab_dev, (uint32_t)a->tab.size(), a->wn,
                                                            a->res, a->src, a->flag, a->req, a->st.dev);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = read_status(ctx, nullptr))) return rc;
        const Status s = *a->st.host();
        if (s.refuse != kNone) return entry_fail(ctx, SVO_ERR_STATE, s.refuse, "subdivide");
        if (!s.n_req) {
            if (s.err != kNone) return entry_fail(ctx, SVO_ERR_STATE, s.err, "subdivide");
            break;
        }
        if (round >= 64) return svo_fail(ctx, SVO_ERR_STATE, "subdivide: chunk loads do not settle");
        std::vector<uint32_t> req(2 * s.n_req);
        HIP_TRY(ctx, hipMemcpy(req.data(), a->req, req.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::vector<std::pair<uint32_t, uint32_t>> first;  // (id, lowest rank)
        for (uint32_t q = 0; q < s.n_req; q++) first.push_back({req[2 * q], req[2 * q + 1]});
        std::sort(first.begin(), first.end());
        for (size_t q = 0; q < first.size(); q++) {
            if (q && first[q].first == first[q - 1].first) continue;
            const uint32_t id = first[q].first, rank = first[q].second;
            if (svo_world_load_chunk(a->world, id) == 0) {
                out->chunks_loaded++;
                if ((rc = mirror_add(ctx, id, rank))) return rc;
            } else {
                table_insert(a->tab, {id, 0, 0, kFailed});
            }
        }
        if ((rc = upload_table(ctx))) return rc;
    }
    // ranks among the successes; flag[n] = 0 makes flag[n] the total after the scan
    HIP_TRY(ctx, hipMemsetAsync(a->flag + n, 0, sizeof(uint32_t), ctx->stream));
    if ((rc = svo_scan_u32(ctx, a->flag, n + 1))) return rc;
    if (a->n_holes)
        sub_popped_kernel<<<svo_div_up(std::min(n, a->n_holes), kThreads), kThreads, 0, ctx->stream>>>(a->holes, a->n_holes, list, n,
                                                                                                       a->flag + n, a->st.dev);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = read_status(ctx, a->flag + n))) return rc;
    const uint32_t done = std::min(a->st.host()->total, limit);
    if (a->st.host()->popped_hit)
        return svo_fail(ctx, SVO_ERR_STATE, "subdivide: an entry lies in a hole group this pass reuses (this list needs the sequential "
                                            "host path, svo_adaptive_subdivide)");
    const uint32_t pops = std::min(done, a->n_holes);
    const uint64_t new_len = uint64_t(a->len) + 8ull * (done - pops);
    if (new_len > ctx->capacity || new_len > kVoxelOff)
        return svo_fail(ctx, SVO_ERR_CAP, "subdivide: " + std::to_string(done) + " subdivisions need " + std::to_string(new_len) +
                                              " words, over the node buffer's capacity of " + std::to_string(ctx->capacity));
    if (done) {
        sub_apply_kernel<<<grid, kThreads, 0, ctx->stream>>>(tree_of(ctx), list, n, a->res, a->src, a->flag, a->holes, a->n_holes,
                                                             a->wn, (uint32_t)ctx->capacity, limit, a->st.dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    a->n_holes -= pops;
    a->len = (uint32_t)new_len;
    out->n_sub = done;
    return SVO_OK;
}

// ---- the unsubdivide pass over the sorted list a->list[1][0, n) ----
int unsubdivide_pass(svo_ctx *ctx, uint32_t n, svo_adaptive_result *out) {
    svo_adapt_state *a = ctx->adapt.get();
    const uint32_t *list = a->list[1], grid = svo_div_up(n, kThreads);
    int rc;
    const size_t words = (a->len + 31) / 32;
    if ((rc = svo_grow(ctx, std::max<size_t>(words, 1), &a->bits))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(a->bits, 0, words * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a->rm, 0xFF, a->rm.size() * sizeof(uint32_t), ctx->stream));
    if ((rc = clear_status(ctx))) return rc;
    unsub_mark_kernel<<<grid, kThreads, 0, ctx->stream>>>(list, n, a->len, a->bits);
    unsub_plan_kernel<<<grid, kThreads, 0, ctx->stream>>>(tree_of(ctx), list, n, a->bits, a->tab_dev, (uint32_t)a->tab.size(),
                                                          a->wn, a->res, a->val, a->src, a->flag, a->rm, a->st.dev);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = read_status(ctx, nullptr))) return rc;
    if (a->st.host()->err != kNone) return entry_fail(ctx, SVO_ERR_STATE, a->st.host()->err, "unsubdivide");
    const bool removals = a->st.host()->removals != 0;
    if (removals) {
        unsub_check_kernel<<<grid, kThreads, 0, ctx->stream>>>(tree_of(ctx), list, n, a->res, a->tab_dev, (uint32_t)a->tab.size(),
                                                               a->wn, a->rm, a->st.dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemsetAsync(a->flag + n, 0, sizeof(uint32_t), ctx->stream));
    if ((rc = svo_scan_u32(ctx, a->flag, n + 1))) return rc;
    if ((rc = read_status(ctx, a->flag + n))) return rc;
    if (a->st.host()->err != kNone) return entry_fail(ctx, SVO_ERR_STATE, a->st.host()->err, "unsubdivide");
    const uint32_t done = a->st.host()->total;
    const size_t hole_room = grown_stack(a->holes.size(), size_t(a->n_holes) + done);
    if ((rc = svo_grow_keep(ctx, hole_room, &a->holes, a->n_holes))) return rc;
    unsub_apply_kernel<<<grid, kThreads, 0, ctx->stream>>>(tree_of(ctx), list, n, a->res, a->val, a->src, a->flag, a->holes,
                                                           a->n_holes, (uint32_t)a->holes.size());
    HIP_TRY(ctx, hipGetLastError());
    a->n_holes += done;
    out->n_unsub = done;
    if (removals) {  // the host world drops them too, so its chunk set stays the host path's
        std::vector<uint32_t> rm(a->tab.size());
        HIP_TRY(ctx, hipMemcpyAsync(rm.data(), a->rm, rm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<Chunk> keep;
        for (size_t s = 0; s < a->tab.size(); s++) {
            if (rm[s] != kNone) {
                svo_world_remove(a->world, a->tab[s].id);
                a->removed.push_back(a->tab[s].id);
            } else {
                keep.push_back(a->tab[s]);
            }
        }
        a->tab.swap(keep);
        if ((rc = upload_table(ctx))) return rc;
    }
    return SVO_OK;
}

// loads that failed in a subdivide pass are forgotten: the next pass may try them again, as the host does; the others
// are resident for every entry from here on.  True when the table changed (the caller uploads it).
bool forget_load_ranks(svo_adapt_state *a) {
    bool changed = false;
    for (const Chunk &c : a->tab) changed |= c.rank != kNone;
    a->tab.erase(std::remove_if(a->tab.begin(), a->tab.end(), [](const Chunk &c) { return c.rank == kFailed; }), a->tab.end());
    for (Chunk &c : a->tab) c.rank = kNone;
    return changed;
}

// One stage of svo_adaptive_expand: the compaction of in[0, n) (its total into st->total), between the events ev[0] and
// ev[1]; the status comes back, which waits for both, and their distance is added to expand_ms[stage].
template <class Keep, class Emit>
int timed_compaction(svo_ctx *ctx, int stage, const uint32_t *in, uint32_t n, Keep keep, Emit emit) {
    svo_adapt_state *a = ctx->adapt.get();
    const uint32_t nt = svo_div_up(n, kTile);
    int rc = svo_grow(ctx, nt + 1, &a->tiles);
    if (rc || (rc = clear_status(ctx))) return rc;
    HIP_TRY(ctx, hipEventRecord(a->ev[0], ctx->stream));
    const Compaction<Keep, Emit> pass{in, keep, emit};
    if ((rc = svo_tile_pass(ctx, pass, pass, nt, nullptr, n, a->tiles, &a->st.dev->total))) return rc;
    HIP_TRY(ctx, hipEventRecord(a->ev[1], ctx->stream));
    if ((rc = read_status(ctx, nullptr))) return rc;
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
    a->expand_ms[stage] += ms;
    return SVO_OK;
}

int check_attached(svo_ctx *ctx) {
    if (!ctx->adapt || !ctx->adapt->world) return svo_fail(ctx, SVO_ERR_STATE, "svo_adaptive_attach not called");
    if (ctx->nodes != ctx->adapt->nodes_at_attach || ctx->capacity != ctx->adapt->capacity)
        return svo_fail(ctx, SVO_ERR_STATE, "the node buffer changed since svo_adaptive_attach: attach again");
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_adaptive_attach(svo_ctx *ctx, svo_world *w, const svo_octree *o) {
    if (!ctx || !w || !o) return SVO_ERR_ARG;
    if (!ctx->store || !ctx->nodes) return svo_fail(ctx, SVO_ERR_STATE, "svo_nodes_alloc / svo_nodes_bind_device not called");
    if (!ctx->scan_clears)
        return svo_fail(ctx, SVO_ERR_STATE, "the device adaptive step needs SVO_OPT_SCAN_CLEARS_COUNTERS=1 (the scan resets the counters)");
    const uint32_t *nodes;
    const float *pos;
    std::vector<uint32_t> holes;
    const size_t len = svo_octree_state(o, &nodes, &pos, holes);
    if (len > ctx->capacity || len > kVoxelOff) return svo_fail(ctx, SVO_ERR_CAP, "the octree is longer than the node buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = svo_workspace_ensure(ctx, ctx->adapt);
    if (rc) return rc;
    svo_adapt_state *a = ctx->adapt.get();
    a->world = nullptr;  // (attached only once everything is up)
    if ((rc = svo_grow(ctx, 3 * ctx->capacity, &a->pos))) return rc;
    a->capacity = ctx->capacity;
    if ((rc = svo_grow(ctx, std::max<size_t>(holes.size() + kListCap, ctx->capacity / 8 + 1), &a->holes))) return rc;
    // (the order behind the store's last write: the plan kernels read the words)
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    if (len) HIP_TRY(ctx, hipMemcpyAsync(a->pos, pos, 3 * len * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (!holes.empty())
        HIP_TRY(ctx, hipMemcpyAsync(a->holes, holes.data(), holes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    a->len = (uint32_t)len;
    a->n_holes = (uint32_t)holes.size();
    a->world = w;
    a->tab.clear();
    if ((rc = rebuild_mirror(ctx, 0))) {
        a->world = nullptr;
        return rc;
    }
    a->nodes_at_attach = ctx->nodes;
    return SVO_OK;
}

int svo_adaptive_step(svo_ctx *ctx, const uint32_t *d_sub, uint32_t n_sub, const uint32_t *d_unsub, uint32_t n_unsub,
                      svo_adaptive_result *out) {
    if (!ctx || !out) return SVO_ERR_ARG;
    if ((d_sub == nullptr) != (d_unsub == nullptr)) return svo_fail(ctx, SVO_ERR_ARG, "give both lists or neither");
    int rc = check_attached(ctx);
    if (rc) return rc;
    svo_adapt_state *a = ctx->adapt.get();
    memset(out, 0, sizeof *out);
    a->removed.clear();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, hipEventRecord(a->ev[0], ctx->stream));
    if (!d_sub) {  // the scan's own lists, clamped like svo_scan_read (adaptive.rs:22,86), their counters reset
        if (!ctx->scan_lists) return svo_fail(ctx, SVO_ERR_STATE, "svo_scan_dispatch not called");
        HIP_TRY(ctx, hipMemcpyAsync(&a->counts_host[0], ctx->scan_sub(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&a->counts_host[1], ctx->scan_unsub(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t lim = (uint32_t)ctx->scan_capacity - 1;
        n_sub = std::min(a->counts_host[0], lim);
        n_unsub = std::min(a->counts_host[1], lim);
        d_sub = ctx->scan_sub() + 1;
        d_unsub = ctx->scan_unsub() + 1;
        HIP_TRY(ctx, hipMemsetAsync(ctx->scan_sub(), 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->scan_unsub(), 0, sizeof(uint32_t), ctx->stream));
    }
    if (n_sub >= kMaxRank || n_unsub >= kMaxRank) return svo_fail(ctx, SVO_ERR_ARG, "at most 2^24 - 1 entries per list");
    if ((rc = grow_entries(ctx, std::max<size_t>(std::max(n_sub, n_unsub), 1) + 1))) return rc;
    if ((rc = svo_build_sort_u32(ctx, d_sub, n_sub, a->list[0]))) return rc;
    if ((rc = svo_build_sort_u32(ctx, d_unsub, n_unsub, a->list[1]))) return rc;
    HIP_TRY(ctx, hipEventRecord(a->ev[1], ctx->stream));
    if (n_sub && (rc = subdivide_pass(ctx, n_sub, kNone, out))) return rc;
    forget_load_ranks(a);
    HIP_TRY(ctx, hipEventRecord(a->ev[2], ctx->stream));
    if ((rc = upload_table(ctx))) return rc;
    if (n_unsub && (rc = unsubdivide_pass(ctx, n_unsub, out))) return rc;
    HIP_TRY(ctx, hipEventRecord(a->ev[3], ctx->stream));
    if ((rc = svo_store_note_write(ctx))) return rc;
    HIP_TRY(ctx, hipEventSynchronize(a->ev[3]));
    for (int k = 0; k < 3; k++) HIP_TRY(ctx, hipEventElapsedTime(&a->ms[k], a->ev[k], a->ev[k + 1]));
    a->ms[3] = float(svo_now_ms() - t0);
    out->length = a->len;
    out->n_removed = (uint32_t)a->removed.size();
    out->removed = a->removed.data();
    return SVO_OK;
}

int svo_adaptive_expand(svo_ctx *ctx, uint32_t max_depth, const float cam[3], float lod_c, uint64_t max_words,
                        svo_adaptive_result *out) {
    if (!ctx || !out) return SVO_ERR_ARG;
    if (max_depth > kMaxTreeDepth) return svo_fail(ctx, SVO_ERR_ARG, "max_depth above 31");
    int rc = check_attached(ctx);
    if (rc) return rc;
    svo_adapt_state *a = ctx->adapt.get();
    if (a->n_holes)  // the host's frontier is then not ascending, and the sorted pass would hand out other groups
        return svo_fail(ctx, SVO_ERR_STATE, "the attached tree has " + std::to_string(a->n_holes) + " free groups in its hole stack: "
                                            "expanding it needs the sequential host path, svo_world_expand");
    memset(out, 0, sizeof *out);
    a->removed.clear();
    memset(a->expand_ms, 0, sizeof a->expand_ms);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(max_words ? max_words : ctx->capacity, ctx->capacity), kVoxelOff);
    View view{};
    view.max_depth = max_depth;
    view.use_cam = cam && lod_c > 0.0f;
    view.lod_c = lod_c;
    if (cam) memcpy(view.cam, cam, sizeof view.cam);
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    float ms = 0.0f;
    uint64_t n_sub = 0;

    // the initial frontier: the leaves of [0, len) (at most len of them)
    uint32_t cur = 0, n_front = 0;
    if (a->len) {
        if ((rc = svo_grow(ctx, a->len, &a->frontier[0]))) return rc;
        if ((rc = timed_compaction(ctx, 0, ctx->nodes, a->len, LeafWord{}, EmitLeaf{tree_of(ctx), a->frontier[0], a->len, a->st.dev}))) return rc;
        if (a->st.host()->err != kNone) return entry_fail(ctx, SVO_ERR_STATE, a->st.host()->err, "expand: leaf");
        n_front = a->st.host()->total;
    }

    // level by level; a level of 2^24 entries or more goes through the pass in consecutive slices (its rank packing)
    uint32_t levels = 0;
    bool full = false;  // the cap leaves no room for another group: the host stops at its next candidate
    while (n_front && !full) {
        levels++;
        const uint32_t nxt = cur ^ 1u;
        const uint64_t room = cap > a->len ? cap - a->len : 0;
        const size_t next_max = std::max<uint64_t>(std::min<uint64_t>(8ull * n_front, room), 8);  // 8 slots per success
        if ((rc = svo_grow(ctx, grown(a->frontier[nxt].size(), next_max), &a->frontier[nxt]))) return rc;
        uint32_t n_next = 0;
        for (uint32_t lo = 0; lo < n_front && !full; lo += kMaxRank - 1u) {
            const uint32_t n = std::min(n_front - lo, kMaxRank - 1u);
            const uint32_t limit = (uint32_t)((cap > a->len ? cap - a->len : 0) / 8u);
            if (!limit) {
                full = true;
                break;
            }
            if ((rc = grow_entries(ctx, grown(a->flag.size(), size_t(n) + 1)))) return rc;
            const uint32_t *front = a->frontier[cur] + lo;
            if ((rc = timed_compaction(ctx, 1, front, n, ViewRefines{a->pos, view}, EmitCandidate{a->list[0]}))) return rc;
            const uint32_t n_cand = a->st.host()->total;
            if (!n_cand) continue;
            const uint32_t len_before = a->len;
            svo_adaptive_result pass{};
            if ((rc = subdivide_pass(ctx, n_cand, limit, &pass))) return rc;
            if (pass.n_sub)
                next_frontier_kernel<<<svo_div_up(n_cand, kThreads), kThreads, 0, ctx->stream>>>(n_cand, a->res, a->flag, limit, len_before,
                                                                                                 a->frontier[nxt] + n_next);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipEventRecord(a->ev[2], ctx->stream));
            if (forget_load_ranks(a) && (rc = upload_table(ctx))) return rc;
            HIP_TRY(ctx, hipEventSynchronize(a->ev[2]));
            HIP_TRY(ctx, hipEventElapsedTime(&ms, a->ev[1], a->ev[2]));
            a->expand_ms[2] += ms;
            n_next += 8u * pass.n_sub;
            n_sub += pass.n_sub;
            out->chunks_loaded += pass.chunks_loaded;
        }
        cur = nxt;
        n_front = n_next;
    }
    if ((rc = svo_store_note_write(ctx))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    a->expand_ms[3] = float(svo_now_ms() - t0);
    a->expand_ms[4] = float(levels);
    out->n_sub = (uint32_t)n_sub;
    out->length = a->len;
    return SVO_OK;
}

int svo_adaptive_expand_timing(svo_ctx *ctx, float ms_out[SVO_ADAPT_EXPAND_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->adapt) return svo_fail(ctx, SVO_ERR_STATE, "svo_adaptive_attach not called");
    memcpy(ms_out, ctx->adapt->expand_ms, sizeof ctx->adapt->expand_ms);
    return SVO_OK;
}

int svo_adaptive_download(svo_ctx *ctx, svo_octree *o) {
    if (!ctx || !o) return SVO_ERR_ARG;
    int rc = check_attached(ctx);
    if (rc) return rc;
    svo_adapt_state *a = ctx->adapt.get();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> nodes(a->len), holes(a->n_holes);
    std::vector<float> pos(3 * size_t(a->len));
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    if (a->len) {
        HIP_TRY(ctx, hipMemcpyAsync(nodes.data(), ctx->nodes, nodes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(pos.data(), a->pos, pos.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (a->n_holes)
        HIP_TRY(ctx, hipMemcpyAsync(holes.data(), a->holes, holes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t &w : nodes) w &= ~15u;  // (counters a trace has raised since the step: the host words carry none)
    svo_octree_assign(o, nodes.data(), pos.data(), a->len, holes.data(), holes.size());
    return SVO_OK;
}

int svo_adaptive_length(svo_ctx *ctx, uint64_t *len_out) {
    if (!ctx || !len_out) return SVO_ERR_ARG;
    int rc = check_attached(ctx);
    if (rc) return rc;
    *len_out = ctx->adapt->len;
    return SVO_OK;
}

int svo_adaptive_timing(svo_ctx *ctx, float ms_out[SVO_ADAPT_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->adapt) return svo_fail(ctx, SVO_ERR_STATE, "svo_adaptive_attach not called");
    memcpy(ms_out, ctx->adapt->ms, sizeof ctx->adapt->ms);
    return SVO_OK;
}

}  // extern "C"

// svo_components.hip -- the connected components of the tree in the node buffer, labelled on the device:
// for every voxel of the listing (svo_list.hip) the rank of the first entry of its component, the component's number and
// the index of its word; and svo_nodes_scatter_device, which writes words at such indices without leaving the device.
// Two entries are linked when the walk of the surface pass (svo_surface.hip), from one of them through one of its six
// faces, stops on the other: the cubes are disjoint, so that is 6-connectivity of the cubes.
//
//   plan      svo_list_plan_count / svo_list_plan_offsets (svo_list.hip), in a plan of the pass's own: the discovery with
//             its checks, the entry counts bottom-up, every group's place in the list and its Morton prefix top-down
//   link      one launch over all groups of the listed levels, one lane per group, as surface_mask_kernel: the group's 8
//             words once, the links between siblings from those registers, the 6 cells beside the group by a
//             dilated-integer step and a walk that resumes on the wave's path in LDS.  The walk goes by index into
//             `order`, not by address: the group below an interior word is first_child[k] plus the interior words before
//             it, so the walk knows start[k] of where it stops, and the rank of the word it stops on is start[k] plus the
//             entries before that word in its group.  Each entry gets at most six ranks (0xFFFFFFFF: no link): an equal-level
//             pair is found from both sides and written from the lower one (its odd face), a coarser neighbour is
//             written from the fine side
//   union     rounds of hook and compress until a round hooks nothing.  hook: for each link (u, v) the roots ru, rv that
//             the round before left; when they differ, atomicMin(&parent[max], min).  compress: every entry chases parent
//             from its old root to the new one.  Parents only ever decrease, so the fixed point is the smallest rank of
//             each component, whatever order the atomics land in: the one place where a tree pass uses atomics
//   ids       svo_scan.h's tile pass over label[i] == i numbers the roots; a gather gives every entry its root's number
//
// No kernel reads, in the launch that writes it, a value another workgroup writes (the eight L2s are not coherent within
// a launch): the hook reads the roots of the launch before and only adds atomics to `parent`; the compress reads `parent`
// and the old roots, and writes the new roots to the other of two arrays.  A compress pass chases at most kChase steps;
// when an entry has not arrived, further passes start from where the entry's old root arrived, so the distance doubles.
// No pointer is checked here: the discovery has checked every pointer in every reachable group before the link pass runs.
// Every error is decided before the first write to the outputs.  The labelling only reads the node buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "svo_ctx.h"
#include "svo_group.h"   // (kThreads, kMaxWords)
#include "svo_morton.h"  // (key_bits, morton_axis_mask, morton_step)
#include "svo_scan.h"    // (the tile pass)

namespace {

constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPathLevels = 21;  // a group's prefix holds at most 20 levels: the groups of the levels 1..21 on a path
constexpr uint32_t kChase = 64;  // steps of one compress pass: pass k reaches (2^k - 1) kChase parents up (8 was measured and was no faster: DESIGN.md 29)
constexpr uint64_t kMaxScatter = 1ull << 31;
enum Status { kStChanged, kStMore, kStTotal, kStWords };
static_assert(kThreads % 64 == 0, "whole waves per workgroup");

// A group's words as masks: bit c of `voxel`: the word is a voxel; of `interior`: it points at a group
struct Masks {
    uint32_t voxel, interior;
};

__device__ inline Masks group_masks(const uint4 &a, const uint4 &b) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    Masks m{0u, 0u};
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        m.voxel |= (w[c] >> 4) > SVO_VOXEL_OFFSET ? 1u << c : 0u;
        m.interior |= (w[c] >> 4) < SVO_VOXEL_OFFSET ? 1u << c : 0u;
    }
    return m;
}

__device__ inline Masks load_masks(const uint32_t *__restrict__ words, uint32_t g) {  // (g a multiple of 8: two aligned 16-byte reads)
    return group_masks(*reinterpret_cast<const uint4 *>(words + g), *reinterpret_cast<const uint4 *>(words + g + 4));
}

// the group below the interior word c of the group with masks m, as an index into order
__device__ inline uint32_t child_group(const Masks &m, uint32_t c, uint32_t first) { return first + __popc(m.interior & ((1u << c) - 1u)); }

// the entries of the listing that lie before word c in its group: a voxel is one, an interior word its group's count
__device__ inline uint32_t entries_before(const Masks &m, uint32_t c, uint32_t first, const uint64_t *__restrict__ cnt) {
    const uint32_t low = (1u << c) - 1u;
    uint32_t e = __popc(m.voxel & low);
    for (uint32_t rest = m.interior & low; rest; rest &= rest - 1u) e += uint32_t(cnt[first++]);
    return e;
}

// The groups order[0, n) of the listed levels, one lane each.  nbr[6 r + f] gets the rank that entry r is linked to
// through face f; the caller has filled nbr with 0xFF bytes.  index_out (or null) gets the entries' word indices.
__global__ __launch_bounds__(kThreads) void components_link_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ order,
                                                                   uint32_t n, const uint32_t *__restrict__ first_child,
                                                                   const uint64_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                                   const uint64_t *__restrict__ key, uint32_t same_value, uint32_t n_list,
                                                                   uint32_t *__restrict__ nbr, uint32_t *__restrict__ index_out) {
    // path[w][j]: the index in order of the group that j levels of the prefix of wave w's first group lead to; [0] is the root group
    __shared__ uint32_t path[kWaves][kPathLevels];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane(blockIdx.x * kThreads + wave * 64u), k = k0 + lane;
    uint64_t lead = 1u;  // the first group's prefix: the same in every lane, so its walk loads through the scalar unit
    if (k0 < n) lead = key[k0];
    const uint32_t lead_levels = key_bits(lead);
    {
        uint32_t at = 0;
        if (lane == 0) path[wave][0] = 0u;
        for (uint32_t j = 0; j < lead_levels; j++) {
            const uint32_t c = uint32_t(lead >> 3u * (lead_levels - 1u - j)) & 7u;
            const Masks m = load_masks(words, order[at]);  // (word c is interior: it lies on the path to a discovered group)
            at = __builtin_amdgcn_readfirstlane(child_group(m, c, first_child[at]));
            if (lane == 0) path[wave][j + 1u] = at;
        }
    }
    __syncthreads();
    if (k >= n) return;

    const uint32_t g = order[k];
    const uint4 lo = *reinterpret_cast<const uint4 *>(words + g), hi = *reinterpret_cast<const uint4 *>(words + g + 4);
    const Masks mine = group_masks(lo, hi);
    const uint32_t vm = mine.voxel;
    if (!vm) return;
    const uint32_t pointer[8] = {lo.x >> 4, lo.y >> 4, lo.z >> 4, lo.w >> 4, hi.x >> 4, hi.y >> 4, hi.z >> 4, hi.w >> 4};
    const uint64_t prefix = key[k];
    const uint32_t levels = key_bits(prefix);  // the words are of level levels + 1
    const uint64_t cell = prefix ^ (1ull << 3u * levels), lead_cell = lead ^ (1ull << 3u * lead_levels);

    // the ranks of the group's voxels; the links between siblings, written from the lower one
    uint32_t rank[8];
    {
        uint32_t r = start[k], child = first_child[k];
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) {
            rank[c] = r;
            if (pointer[c] > SVO_VOXEL_OFFSET) {
                r++;
            } else if (pointer[c] < SVO_VOXEL_OFFSET) {
                if (vm >> (c + 1u)) r += uint32_t(cnt[child]);  // (a voxel follows: the entries below this word lie before it)
                child++;
            }
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        if (!(vm >> c & 1u) || rank[c] >= n_list) continue;  // (never the latter: n_list is the root's count)
        if (index_out) index_out[rank[c]] = g + c;
#pragma unroll
        for (uint32_t axis = 0; axis < 3; axis++) {
            const uint32_t bit = 4u >> axis, other = c | bit;
            if ((c & bit) || !(vm >> other & 1u)) continue;
            if (same_value && pointer[c] != pointer[other]) continue;
            nbr[6ull * rank[c] + 2u * axis + 1u] = rank[other];
        }
    }

    // the 6 cells beside the group
    for (uint32_t f = 0; f < 6; f++) {
        const uint32_t axis = f >> 1, up = f & 1u, bit = 4u >> axis;
        const uint32_t side = (axis == 0 ? 0x0Fu : axis == 1 ? 0x33u : 0x55u) << (up ? bit : 0u);  // the children at that face
        if (!(vm & side)) continue;
        const uint64_t mask = morton_axis_mask(axis, levels);
        if ((cell & mask) == (up ? mask : 0u)) continue;  // the cell lies outside the grid (always, for the root group)
        const uint64_t to = morton_step(cell, mask, up);
        // the levels that `to` shares with the first group's path
        const uint32_t d = min(levels, lead_levels);
        const uint64_t x = (to >> 3u * (levels - d)) ^ (lead_cell >> 3u * (lead_levels - d));
        uint32_t j = x ? d - 1u - (63u - (uint32_t)__clzll((long long)x)) / 3u : d;
        uint32_t at = path[wave][j];
        for (;; j++) {
            const uint32_t group = order[at];
            const Masks m = load_masks(words, group);
            const uint32_t first = first_child[at];
            if (j == levels) {  // the neighbour is a group of this level: each pair is written from its lower voxel
                if (up) {
                    const uint32_t pairs = vm & side & (m.voxel << bit);  // bit c: child c and the voxel c ^ bit behind its face
#pragma unroll
                    for (uint32_t c = 0; c < 8; c++) {
                        const uint32_t other = c ^ bit;
                        if (!(pairs >> c & 1u)) continue;
                        if (same_value && pointer[c] != words[group + other] >> 4) continue;
                        if (rank[c] < n_list) nbr[6ull * rank[c] + f] = start[at] + entries_before(m, other, first, cnt);
                    }
                }
                break;
            }
            const uint32_t c = uint32_t(to >> 3u * (levels - 1u - j)) & 7u;
            if (!(m.interior >> c & 1u)) {  // a coarser voxel links all four, the empty word none
                if (m.voxel >> c & 1u) {
                    const uint32_t p = words[group + c] >> 4, r = start[at] + entries_before(m, c, first, cnt);
#pragma unroll
                    for (uint32_t q = 0; q < 8; q++) {
                        if (!((vm & side) >> q & 1u)) continue;
                        if (same_value && pointer[q] != p) continue;
                        if (rank[q] < n_list) nbr[6ull * rank[q] + f] = r;
                    }
                }
                break;
            }
            at = child_group(m, c, first);
        }
    }
}

__global__ __launch_bounds__(kThreads) void components_init_kernel(uint32_t n, uint32_t *__restrict__ parent, uint32_t *__restrict__ root) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    root[i] = i;
}

// One lane per entry.  root holds what the launch before left and is only read; parent only receives atomics, at roots.
__global__ __launch_bounds__(kThreads) void components_hook_kernel(const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ root,
                                                                   uint32_t n, uint32_t *parent, uint32_t *changed) {
    const uint32_t u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= n) return;
    const uint32_t ru = root[u];
    bool any = false;
#pragma unroll
    for (uint32_t f = 0; f < 6; f++) {
        const uint32_t v = nbr[6ull * u + f];
        if (v >= n) continue;  // (0xFFFFFFFF: no link)
        const uint32_t rv = root[v];
        if (ru == rv) continue;
        atomicMin(&parent[max(ru, rv)], min(ru, rv));
        any = true;
    }
    if (any) *changed = 1u;  // (every writer stores the same value)
}

// One lane per entry: from in[i], or with `jump` from in[in[i]], up to kChase parents up, into out[i].  Every value that
// in holds for an entry is an ancestor of it, and parent is only read here.
__global__ __launch_bounds__(kThreads) void components_compress_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ in,
                                                                       uint32_t *__restrict__ out, uint32_t n, uint32_t jump, uint32_t *more) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t r = in[i];
    if (jump) r = in[r];
    uint32_t p = parent[r];
    for (uint32_t s = 0; s < kChase && p != r; s++) {  // (parents descend: the chase ends)
        r = p;
        p = parent[r];
    }
    out[i] = r;
    if (p != r) *more = 1u;
}

// The numbering's items: 16 labels per thread as the mask of those that are roots.
struct Roots {
    const uint32_t *label;
    __device__ uint32_t load(uint32_t i0, uint32_t m) const {
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
            if (i0 + j < m && label[i0 + j] == i0 + j) bits |= 1u << j;
        return bits;
    }
    __device__ uint32_t count(uint32_t bits) const { return __popc(bits); }
};

struct RootNumbers {
    uint32_t *number;  // per entry; written at the roots
    __device__ void operator()(const Roots &, uint32_t i0, uint32_t bits, uint32_t rank) const {
        for (; bits; bits &= bits - 1u) number[i0 + (uint32_t)__ffs(bits) - 1u] = rank++;
    }
};

__global__ __launch_bounds__(kThreads) void components_id_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ number,
                                                                 uint32_t n, uint32_t *__restrict__ id_out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) id_out[i] = number[label[i]];
}

// words[i], or `fill` without words, to nodes[index[i]]; an index behind the tree is skipped
__global__ __launch_bounds__(kThreads) void scatter_device_kernel(uint32_t *__restrict__ nodes, uint32_t n_words, const uint32_t *__restrict__ index,
                                                                  const uint32_t *__restrict__ words, uint32_t fill, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = index[i];
    if (at < n_words) nodes[at] = words ? words[i] : fill;
}

enum Ev { kEvStart, kEvPlan, kEvLink, kEvUnion, kEvIds, kEvFill, kEvs };

}  // namespace

// Per-context workspace of the labelling (svo_ctx::components): a listing plan of its own, 24 bytes of links and 12 of
// parents and roots per list entry, the tile sums.
struct svo_components_state {
    svo_list_plan plan;
    svo_dev<uint32_t> nbr, parent, root_a, root_b, tile_sum;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_COMPONENTS_TIMES> timer;
    uint32_t rounds = 0;  // of the last call that ran

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        if (int rc = plan.create(ctx)) return rc;
        return status.alloc(ctx, kStWords);
    }
};

extern "C" {

int svo_nodes_label_components(svo_ctx *ctx, const svo_components_params *p, uint32_t *label_out_dev, uint32_t *id_out_dev,
                               uint32_t *index_out_dev, uint64_t *n_out, uint64_t *n_components_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out || !n_components_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out or n_components_out");
    int rc = svo_check_flags(ctx, p->flags, SVO_COMPONENTS_SAME_VALUE);
    if (rc || (rc = svo_check_depth(ctx, p->depth, 21))) return rc;
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t n_words = (uint32_t)std::min<uint64_t>(p->n_words, kMaxWords), depth = p->depth;
    if ((rc = svo_workspace_ensure(ctx, ctx->components))) return rc;
    svo_components_state *s = ctx->components.get();
    if ((rc = s->plan.grow(ctx, n_words / 8)) || (rc = s->timer.begin(ctx))) return rc;

    // the passes read the words: behind every earlier write to the store, whichever context issued it
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    if ((rc = svo_list_plan_count(ctx, &s->plan, p->n_words, depth, false, nullptr))) return rc;
    const svo_list_plan &pl = s->plan;
    const uint32_t n = (uint32_t)pl.count, n_tiles = svo_div_up(n, kTile), grid = svo_div_up(n, kThreads);  // (below 2^31: the plan refused more)
    if (label_out_dev && pl.count > p->max_entries)
        return svo_fail(ctx, SVO_ERR_CAP, "the list has " + std::to_string(pl.count) + " entries, more than max_entries = " +
                                              std::to_string(p->max_entries));
    uint32_t rounds = 0, total = 0;
    uint32_t *label = nullptr, *spare = nullptr;
    if (n) {
        if ((rc = svo_grow(ctx, 6 * (size_t)n, &s->nbr)) || (rc = svo_grow(ctx, (size_t)n, &s->parent, &s->root_a, &s->root_b)) ||
            (rc = svo_grow(ctx, (size_t)n_tiles, &s->tile_sum)))
            return rc;
        if ((rc = svo_list_plan_offsets(ctx, &s->plan, depth, false))) return rc;
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvPlan));

    if (n) {
        const uint32_t m = pl.walk.level_off[pl.listed];
        HIP_TRY(ctx, hipMemsetAsync(s->nbr, 0xFF, 6 * (size_t)n * sizeof(uint32_t), ctx->stream));
        components_link_kernel<<<svo_div_up(m, kThreads), kThreads, 0, ctx->stream>>>(
            ctx->nodes, pl.walk.order, m, pl.walk.first_child, pl.cnt, pl.start, pl.key, p->flags & SVO_COMPONENTS_SAME_VALUE ? 1u : 0u, n,
            s->nbr, label_out_dev ? index_out_dev : nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvLink));

    if (n) {
        label = s->root_a, spare = s->root_b;
        const uint32_t *st = s->status.host();
        components_init_kernel<<<grid, kThreads, 0, ctx->stream>>>(n, s->parent, label);
        for (bool changed = true; changed; rounds++) {
            HIP_TRY(ctx, s->status.zero(ctx));
            components_hook_kernel<<<grid, kThreads, 0, ctx->stream>>>(s->nbr, label, n, s->parent, s->status.dev + kStChanged);
            for (uint32_t jump = 0;; jump = 1) {
                components_compress_kernel<<<grid, kThreads, 0, ctx->stream>>>(s->parent, label, spare, n, jump, s->status.dev + kStMore);
                HIP_TRY(ctx, hipGetLastError());
                std::swap(label, spare);
                if ((rc = s->status.read(ctx))) return rc;
                if (!st[kStMore]) break;
                HIP_TRY(ctx, hipMemsetAsync(s->status.dev + kStMore, 0, sizeof(uint32_t), ctx->stream));
            }
            changed = st[kStChanged] != 0;
        }
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvUnion));

    if (n) {
        const Roots roots{label};
        if ((rc = svo_tile_count(ctx, roots, n_tiles, nullptr, n, s->tile_sum, s->status.dev + kStTotal))) return rc;
        if ((rc = s->status.read(ctx))) return rc;
        total = s->status.host()[kStTotal];
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvIds));

    if (label_out_dev && n) {
        HIP_TRY(ctx, hipMemcpyAsync(label_out_dev, label, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        if (id_out_dev) {
            tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(Roots{label}, RootNumbers{spare}, nullptr, n, s->tile_sum);
            components_id_kernel<<<grid, kThreads, 0, ctx->stream>>>(label, spare, n, id_out_dev);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvFill));
    *n_out = n;
    *n_components_out = total;
    s->rounds = rounds;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_components_timing(svo_ctx *ctx, float ms_out[SVO_COMPONENTS_TIMES], uint32_t *rounds_out) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->components) return svo_fail(ctx, SVO_ERR_STATE, "no components labelled on this context yet");
    if (rounds_out) *rounds_out = ctx->components->rounds;
    return ctx->components->timer.read(ctx, ms_out);
}

int svo_nodes_scatter_device(svo_ctx *ctx, const uint32_t *index_dev, const uint32_t *words_dev, uint32_t fill, size_t n,
                             uint64_t n_words) {
    if (!ctx) return SVO_ERR_ARG;
    if (n && !index_dev) return svo_fail(ctx, SVO_ERR_ARG, "null index_dev");
    if (n >= kMaxScatter) return svo_fail(ctx, SVO_ERR_ARG, "n must be below 2^31 (got " + std::to_string(n) + ")");
    int rc;
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, n_words))) return rc;
    if (!n) return SVO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // a shared store: writes land in the order they were issued, whichever context issued them
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    scatter_device_kernel<<<svo_div_up(n, kThreads), kThreads, 0, ctx->stream>>>(
        ctx->nodes, (uint32_t)std::min<uint64_t>(n_words, kMaxWords), index_dev, words_dev, fill, (uint32_t)n);
    HIP_TRY(ctx, hipGetLastError());
    return svo_store_note_write(ctx);
}

}  // extern "C"
